"""The rule of the 16-bit feature rows, restated in CPU torch: upcast the float16 / bfloat16 rows to float32,
apply the float32 op's documented expression -- one IEEE float32 operation per torch call, in the kernels' order, nothing
contracted -- and round ONCE to the type with ``.to(T)`` (to nearest, ties to even, denormals kept, overflow to inf, NaN stays
NaN: tests/test_rows16.py pins that behaviour of ``.to``). With ``T = torch.float32`` the last step is the identity and the
functions restate the float32 ops themselves.

Everything takes and returns CPU tensors. Pure moves return the element's own bits.
"""
import torch

TYPES = (torch.float16, torch.bfloat16)
MANTISSA_BITS = {torch.float16: 10, torch.bfloat16: 7}     # explicit mantissa bits: 1 + 2^-bits is the neighbour of 1


def rn(x32, dtype):
    """the one rounding"""
    assert x32.dtype == torch.float32
    return x32.to(dtype)


def same_bits(a, b):
    """equal shape and type, NaN in the same positions, every other element bit for bit (so -0 differs from +0)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    ints = {2: torch.int16, 4: torch.int32}[a.element_size()]
    return torch.equal(a.view(ints)[~na], b.view(ints)[~nb])


def group_linear(xyz, new_xyz, z, idx, w_xyz, bias=None):
    """out[b,co,m,s] = RN((z[b,co,idx] + (w0*dx + w1*dy + w2*dz)) + bias[co]), (dx,dy,dz) = xyz[b,idx[b,m,s]] - new_xyz[b,m]"""
    b, c, n = z.shape
    m, ns = idx.shape[1], idx.shape[2]
    z32, ix = z.float(), idx.long()
    out = torch.empty((b, c, m, ns), dtype=torch.float32)
    for k in range(b):
        d = xyz[k][ix[k]] - new_xyz[k][:, None, :]                     # (m, ns, 3)
        dx, dy, dz = d[..., 0][None], d[..., 1][None], d[..., 2][None]    # (1, m, ns)
        w0, w1, w2 = (w_xyz[:, j].reshape(c, 1, 1) for j in range(3))
        t = (w0 * dx + w1 * dy) + w2 * dz
        v = z32[k][:, ix[k]] + t
        if bias is not None:
            v = v + bias.reshape(c, 1, 1)
        out[k] = v
    return rn(out, z.dtype)


def pool_max(x):
    """(rows, ns) -> (values (rows), arg (rows) int32): a NaN outranks everything (the first one), otherwise the largest value at
    its lowest position; -0 == +0 is a tie. The value is the winning element itself."""
    x32 = x.float()
    rows, ns = x32.shape
    nan = torch.isnan(x32)
    pos = torch.arange(ns).expand(rows, ns)
    first_nan = torch.where(nan, pos, torch.full_like(pos, ns)).min(dim=1).values
    clean = torch.where(nan, torch.full_like(x32, float("-inf")), x32)
    top = clean.max(dim=1, keepdim=True).values
    first_top = torch.where(clean == top, pos, torch.full_like(pos, ns)).min(dim=1).values
    arg = torch.where(first_nan < ns, first_nan, first_top)
    return x[torch.arange(rows), arg], arg.to(torch.int32)


def pool_max_grad(grad_out, arg, ns):
    """(rows), (rows) -> (rows, ns): grad_out[row] at arg[row], +0 elsewhere"""
    rows = grad_out.shape[0]
    g = torch.zeros((rows, ns), dtype=grad_out.dtype)
    g[torch.arange(rows), arg.long()] = grad_out
    return g


def three_interpolate(points, idx, weight):
    """out[b,c,i] = RN((w0 * p[i0] + w1 * p[i1]) + w2 * p[i2])"""
    b, c, m = points.shape
    p32, ix = points.float(), idx.long()
    out = torch.empty((b, c, idx.shape[1]), dtype=torch.float32)
    for k in range(b):
        p0, p1, p2 = (p32[k][:, ix[k, :, j]] for j in range(3))         # (c, n)
        w0, w1, w2 = (weight[k, :, j][None] for j in range(3))
        out[k] = (w0 * p0 + w1 * p1) + w2 * p2
    return rn(out, points.dtype)


def gather(features, idx):
    """(B,C,N), (B,M) -> (B,C,M), a move"""
    return torch.stack([features[k][:, idx[k].long()] for k in range(features.shape[0])])


def grouping(features, idx):
    """(B,C,N), (B,M,ns) -> (B,C,M,ns), a move"""
    return torch.stack([features[k][:, idx[k].long()] for k in range(features.shape[0])])


def scatter_rows(grad, idx, n):
    """the gradient of gather / grouping: (B,C,...) summed into (B,C,N) at idx, in float32, index order, rounded once. The tests
    feed values whose float32 sums are exact, so the order of the summation does not show."""
    b, c = grad.shape[0], grad.shape[1]
    g32 = grad.float().reshape(b, c, -1)
    out = torch.zeros((b, c, n), dtype=torch.float32)
    for k in range(b):
        out[k].index_add_(1, idx[k].reshape(-1).long(), g32[k])
    return rn(out, grad.dtype)


def three_interpolate_grad(grad, idx, weight, m):
    """(B,C,n) -> (B,C,m): grad * w_j summed at idx_j (exact sums in the tests, as scatter_rows)"""
    b, c, n = grad.shape
    g32 = grad.float()
    out = torch.zeros((b, c, m), dtype=torch.float32)
    for k in range(b):
        for j in range(3):
            out[k].index_add_(1, idx[k, :, j].long(), g32[k] * weight[k, :, j][None])
    return rn(out, grad.dtype)


def group_linear_grad_w(grad, xyz, new_xyz, idx):
    """(B,C,M,ns) -> (C,3) float32: sum of grad * (xyz[idx] - centre) (exact sums in the tests)"""
    b, c = grad.shape[0], grad.shape[1]
    g32 = grad.float()
    out = torch.zeros((c, 3), dtype=torch.float32)
    for k in range(b):
        d = xyz[k][idx[k].long()] - new_xyz[k][:, None, :]               # (m, ns, 3)
        out += torch.einsum("cms,msj->cj", g32[k].double(), d.double()).float()
    return out
