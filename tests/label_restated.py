"""The label path of the reference restated on the CPU oracle (test infrastructure only).

Written from the rule the reference's ``_warp_label`` / ``_init_y_label`` / ``_resample_inplane``
follow (unires/_core.py:402-492): for every distinct label value u, ascending, a linear pull of
the indicator (label == u) with zero bound and the in-FOV mask; u wins where its pull beats the
best so far strictly, and the best starts at 0.  tests/test_label.py pins these against the
reference's own functions where its sources are at hand.
"""
import torch

from oracle import nitorch_restated as N


def warp_label(label, grid, p_of=None):
    """(labels, best probability[, probability of the value ``p_of`` holds at each voxel]).

    ``grid``: dense (X, Y, Z, 3) voxel coordinates into ``label``."""
    u = label.unique()
    if u.numel() > 255:
        raise ValueError('Too many label values.')
    f = torch.zeros(grid.shape[:3], dtype=label.dtype)
    p = torch.zeros(grid.shape[:3], dtype=torch.float32)
    q = torch.zeros(grid.shape[:3], dtype=torch.float32) if p_of is not None else None
    for v in u:
        t = N.grid_pull((label == v).float()[None, None], grid[None], interpolation=1, bound='zero',
                        extrapolate=False)[0, 0]
        m = t > p
        p[m] = t[m]
        f[m] = v
        if q is not None:
            q = torch.where(p_of == v, t, q)
    return (f, p) if q is None else (f, p, q)


def affine_grid(mat, shape):
    """The reference's grid: the float64 affine cast to float32, then lin @ ijk + off."""
    return N.affine_grid(torch.as_tensor(mat).to(torch.float32), tuple(int(s) for s in shape))


def init_y_label(x, y):
    """y[c].label from x[c][0].label (only the first repeat is looked at)."""
    dim_y, mat_y = tuple(y[0].dim), torch.as_tensor(y[0].mat, dtype=torch.float64)
    for c in range(len(x)):
        if x[c][0].label is not None:
            mat = torch.linalg.solve(torch.as_tensor(x[c][0].mat, dtype=torch.float64), mat_y)
            y[c].label = warp_label(x[c][0].label[0], affine_grid(mat, dim_y))[0]
    return y


def resample_plan(mat_x, dim_x, vx):
    """(D, new dim) of the in-plane resampling, or None when the image is skipped."""
    I = torch.eye(4, dtype=torch.float64)
    vx_x = N.voxel_size(torch.as_tensor(mat_x, dtype=torch.float64))
    D = I.clone()
    for i in range(3):
        D[i, i] = (vx[i] if isinstance(vx, (list, tuple)) else vx) / vx_x[i]
        if D[i, i] < 1.0:
            D[i, i] = 1
    if float((I - D).abs().sum()) < 1e-4:
        return None
    dim = torch.as_tensor(dim_x, dtype=torch.float64)
    return D, tuple(D[:3, :3].inverse().mm(dim[:, None]).floor().squeeze().int().tolist())


def resample_inplane(x, force_inplane_res, max_iter, vx):
    """Nearest-neighbour data, warped labels, updated mat / dim (in place on x)."""
    if not (force_inplane_res and max_iter > 0):
        return x
    for xc in x:
        for xn in xc:
            plan = resample_plan(xn.mat, xn.dim, vx)
            if plan is None:
                continue
            D, dim = plan
            grid = affine_grid(D, dim)
            xn.dat = N.grid_pull(xn.dat[None, None], grid[None], interpolation=0, bound='zero',
                                 extrapolate=False)[0, 0]
            if xn.label is not None:
                xn.label[0] = warp_label(xn.label[0], grid)[0]
            xn.mat = torch.as_tensor(xn.mat, dtype=torch.float64).matmul(D)
            xn.dim = dim
    return x


def voronoi_labels(shape, values, gen, device='cpu'):
    """Voronoi parcellation of ``shape``: each voxel takes the value of its nearest seed (float32,
    on ``device``; the seeds come from the CPU generator ``gen``)."""
    values = torch.as_tensor(values, dtype=torch.float32).to(device)
    seeds = (torch.rand(len(values), 3, generator=gen, dtype=torch.float64) *
             torch.tensor(shape, dtype=torch.float64)).to(device)
    ax = [torch.arange(n, dtype=torch.float64, device=device) for n in shape]
    pts = torch.stack(torch.meshgrid(*ax, indexing='ij'), -1).reshape(-1, 3)
    near = torch.empty(pts.shape[0], dtype=torch.long, device=device)
    for a in range(0, pts.shape[0], 1 << 18):
        near[a:a + (1 << 18)] = torch.cdist(pts[a:a + (1 << 18)], seeds).argmin(1)
    return values[near].reshape(shape)
