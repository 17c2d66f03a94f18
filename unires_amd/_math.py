"""The two nitorch scalar helpers ``_format_y`` calls (unires/_core.py:13,17,203-207,244-245),
restated on torch  [recalled]."""
import torch


def round(t, decimals=0):
    """nitorch.core.math.round: rounding to ``decimals`` decimal places."""
    return torch.round(torch.as_tensor(t) * 10 ** decimals) / 10 ** decimals


def ceil_pow(t, p=2.0, l=2.0, mx=None):
    """nitorch.core.utils.ceil_pow: per element the smallest l * p**n (n = 0, 1, ...) that is
    >= t, so at least l, clipped to ``mx`` where one is given.  A new tensor of t's dtype."""
    t = torch.as_tensor(t)
    out = []
    for v in t.reshape(-1).tolist():
        c = float(l)
        while c < v:
            c *= p
        out.append(min(c, float(mx)) if mx else c)
    return torch.tensor(out, dtype=t.dtype, device=t.device).reshape(t.shape)
