"""Multi-contrast phantoms for the coregistration tests: one anatomy of labelled ellipsoids defined in
world coordinates (mm), an intensity map per contrast that is not monotonic in the label, Gaussian
noise, thick slices averaged over sub-slices, and planted rigid misalignments of the headers."""
import numpy as np
import torch

# (centre mm, radii mm, rotation about z rad, label); later ellipsoids overwrite earlier ones
ELLIPSOIDS = [((0, 0, 0), (62, 74, 60), 0.0, 1), ((0, 0, 4), (54, 66, 52), 0.1, 2),
              ((-18, 10, 8), (16, 28, 20), 0.4, 3), ((20, 8, 6), (14, 24, 22), -0.3, 4),
              ((0, -32, -10), (22, 12, 14), 0.0, 5), ((4, 22, -22), (10, 10, 16), 0.7, 6),
              ((-6, -6, 20), (8, 18, 8), -0.5, 7)]
CONTRASTS = [[0, 300, 900, 1500, 600, 1200, 200, 1800],
             [0, 1400, 500, 200, 1100, 700, 1600, 300],
             [0, 700, 1500, 400, 200, 1700, 900, 1200]]


def labels(w, scale=1.0):
    """Labels at world points w (..., 3) float32 torch; the anatomy is shrunk by ``scale``."""
    if scale != 1.0:
        w = w / scale
    lab = torch.zeros(w.shape[:-1], dtype=torch.int64, device=w.device)
    for c, r, th, k in ELLIPSOIDS:
        d = w - torch.tensor(c, dtype=w.dtype, device=w.device)
        cs, sn = np.cos(th), np.sin(th)
        u = cs * d[..., 0] + sn * d[..., 1]
        v = -sn * d[..., 0] + cs * d[..., 1]
        inside = (u / r[0]) ** 2 + (v / r[1]) ** 2 + (d[..., 2] / r[2]) ** 2 <= 1.0
        lab[inside] = k
    return lab


def true_mat(dim, vx):
    m = np.diag(list(vx) + [1.0])
    m[:3, 3] = -(np.asarray(dim) - 1) / 2.0 * np.asarray(vx)
    return m


def observation(dim, vx, contrast, seed, device, sub_axis=None, sub=4, noise=75.0, scale=1.0, rician=False):
    """float32 (dim) volume of the phantom seen with a (dim, vx) grid centred on the origin; a thick
    axis (sub_axis) averages `sub` sub-slices.  Returns (dat, true voxel-to-world)."""
    mat = true_mat(dim, vx)
    ax = [torch.arange(n, dtype=torch.float32, device=device) for n in dim]
    ijk = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1)
    lut = torch.tensor(CONTRASTS[contrast], dtype=torch.float32, device=device)
    offs = [0.0] if sub_axis is None else [(k + 0.5) / sub - 0.5 for k in range(sub)]
    acc = torch.zeros(tuple(dim), dtype=torch.float32, device=device)
    A = torch.tensor(mat[:3, :3], dtype=torch.float32, device=device)
    b = torch.tensor(mat[:3, 3], dtype=torch.float32, device=device)
    for o in offs:
        p = ijk.clone()
        if sub_axis is not None:
            p[..., sub_axis] += o
        acc += lut[labels(p @ A.T + b, scale)]
    acc /= len(offs)
    g = torch.Generator(device='cpu').manual_seed(seed)
    n1 = noise * torch.randn(tuple(dim), generator=g).to(device)
    if rician:  # the magnitude of complex Gaussian noise, as MRI magnitude images carry
        n2 = noise * torch.randn(tuple(dim), generator=g).to(device)
        return torch.sqrt((acc + n1) ** 2 + n2 ** 2), mat
    return acc + n1, mat


def random_rigid(rng, trans=5.0, rot=0.1):
    from unires_amd._rigid import _expm, affine_basis
    q = np.concatenate([rng.uniform(-trans, trans, 3), rng.uniform(-rot, rot, 3)])
    return _expm(q, affine_basis()).numpy()


def rms_mm(mat_found, mat_true, dim, stride=4, scale=1.0):
    """RMS distance (mm) between where mat_found and mat_true put the voxels of the foreground
    (label > 0, on a stride grid)."""
    ax = [np.arange(0, n, stride, dtype=np.float64) for n in dim]
    ijk = np.stack(np.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    h = np.concatenate([ijk, np.ones((len(ijk), 1))], 1)
    wt = h @ np.asarray(mat_true).T
    fg = labels(torch.as_tensor(wt[:, :3], dtype=torch.float32), scale).numpy() > 0
    wf = h[fg] @ np.asarray(mat_found).T
    return float(np.sqrt(np.mean(np.sum((wf - wt[fg])[:, :3] ** 2, 1))))
