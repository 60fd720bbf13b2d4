"""The 16-bit feature rows on the GPU, bit for bit against the restatement of the rule (tests/rows16_restate.py): the native
kernels of csrc/rows16.hip on every path their launchers choose -- staged and scalar, 16-byte, 8-byte and element-wise, with
base pointers 0, 1 and 3 elements off a 16-byte boundary (guarded as tests/offset_alloc.py guards its tensors, and checked by
its ``check()``) -- and the ops that take the upcast route. NaN is compared by position, everything else by its 16 bits."""
import functools

import numpy as np
import pytest
import torch

import offset_alloc
import rows16_restate as R
from conftest import CANARY, GUARD_BYTES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
OFFSETS = (0, 1, 3)           # elements
SENTINEL_BITS = 0x5A5A        # float16 203.25, bfloat16 1.5e16: no case computes it


def at_offset(values_or_shape, dtype, off):
    """a contiguous device tensor whose data pointer sits `off` elements past a 16-byte boundary, canaries on both sides;
    a shape gives an output prefilled with the sentinel. Registered with offset_alloc, whose check() reads the canaries."""
    values = values_or_shape if isinstance(values_or_shape, torch.Tensor) else None
    shape = tuple(values.shape) if values is not None else tuple(int(v) for v in values_or_shape)
    size = torch.empty((), dtype=dtype).element_size()
    nbytes = int(np.prod(shape, dtype=np.int64)) * size
    pad = (-nbytes) % 16 + 16
    raw = torch.full((GUARD_BYTES + nbytes + pad + GUARD_BYTES,), CANARY, dtype=torch.uint8, device=DEV)
    start = GUARD_BYTES + off * size
    body = torch.empty((0,), dtype=dtype, device=DEV).set_(raw.untyped_storage(), start // size, shape)
    assert body.is_contiguous() and body.data_ptr() % 16 == (off * size) % 16
    if values is not None:
        body.copy_(values.to(dtype))
    else:
        body.view(torch.int16 if size == 2 else torch.int32).fill_(SENTINEL_BITS)
    offset_alloc._live.append((raw, start, nbytes, shape, dtype))
    return body


def same(got, want):
    return R.same_bits(got, want)


def ext():
    from epnet_amd import pointnet2_cuda
    return pointnet2_cuda


# ---- group_linear -----------------------------------------------------------------------------------------------------
GL_CASES = {            # (b, c, n, npoint, ns)
    "partial_chunk": (2, 5, 1000, 8, 4),
    "chunks_odd_n": (2, 70, 1001, 8, 4),
    "row_32k": (1, 4, 16384, 4, 16),
    "beyond_lds": (1, 2, 32776, 4, 4),
    "ns3": (2, 3, 64, 5, 3),
}


@functools.lru_cache(maxsize=None)
def gl_case(name, tname, with_bias):
    b, c, n, m, ns = GL_CASES[name]
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(11 + len(name))
    xyz = torch.randn((b, n, 3), generator=g)
    new_xyz = xyz[:, torch.randperm(n, generator=g)[:m]].clone()
    z = (torch.randn((b, c, n), generator=g) * 4).to(dtype)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    idx[:, 0, 0], idx[:, 0, 1], idx[:, 0, 2] = 0, n - 1, n - 1          # both ends and a repeat
    idx[:, 1] = idx[:, 1, 0:1]                                         # a padded neighbour list: one index ns times
    w = torch.randn((c, 3), generator=g)
    bias = torch.randn((c,), generator=g) if with_bias else None
    want = R.group_linear(xyz, new_xyz, z, idx, w, bias)
    return xyz, new_xyz, z, idx, w, bias, want


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", list(GL_CASES))
def test_group_linear(name, tname, with_bias, off):
    b, c, n, m, ns = GL_CASES[name]
    dtype = TYPES[tname]
    xyz, new_xyz, z, idx, w, bias, want = gl_case(name, tname, with_bias)
    zd, out = at_offset(z, dtype, off), at_offset((b, c, m, ns), dtype, off)
    ext().group_linear_h_wrapper(b, c, n, m, ns, xyz.to(DEV), new_xyz.to(DEV), zd, idx.to(DEV), w.to(DEV),
                                 None if bias is None else bias.to(DEV), out)
    offset_alloc.check()
    assert same(out, want)


@pytest.mark.parametrize("ns", [4, 3])          # the staged kernel's packed conversion and the scalar kernel's single one
@pytest.mark.parametrize("tname", list(TYPES))
def test_group_linear_rounds_once_to_nearest_even(tname, ns):
    """w_xyz = 0, so out = RN(z + bias): both ties, denormals in and out, overflow, NaN"""
    dtype = TYPES[tname]
    bits = R.MANTISSA_BITS[dtype]
    eps = 2.0 ** -(bits + 1)                                   # half the distance from 1 to its neighbour
    tiny = 2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -24      # the smallest denormal of T
    big, big_bias = (3e38, 1e38) if dtype == torch.bfloat16 else (60000.0, 60000.0)
    zrow = torch.tensor([1.0, 1.0 + 2 * eps, tiny, big, 0.0, -1.0, float("nan"), -tiny]).to(dtype)
    assert zrow[2].item() == tiny and zrow[1].item() == 1.0 + 2 * eps
    c, n = 4, 8
    z = zrow.expand(1, c, n).contiguous()
    bias = torch.tensor([eps, 0.0, big_bias, 1.5 * tiny], dtype=torch.float32)
    m = 2
    idx = torch.arange(n, dtype=torch.int32).repeat(2)[: m * ns].reshape(1, m, ns).contiguous()
    idx[0, 1, : min(ns, 4)] = torch.tensor([3, 4, 6, 7][: min(ns, 4)], dtype=torch.int32)
    xyz = torch.randn((1, n, 3), generator=torch.Generator().manual_seed(1))
    new_xyz = xyz[:, :m].clone()
    w = torch.zeros((c, 3))
    want = R.group_linear(xyz, new_xyz, z, idx, w, bias)
    out = at_offset((1, c, m, ns), dtype, 0)
    ext().group_linear_h_wrapper(1, c, n, m, ns, xyz.to(DEV), new_xyz.to(DEV), z.to(DEV), idx.to(DEV), w.to(DEV), bias.to(DEV), out)
    offset_alloc.check()
    got = out.cpu()
    # the literal answers for the first position's neighbours 0, 1, 2 (z = 1, 1 + 2 eps, tiny)
    assert got[0, 0, 0, 0].item() == 1.0                       # 1 + eps: a tie, to even = down
    assert got[0, 0, 0, 1].item() == 1.0 + 4 * eps             # 1 + 3 eps: a tie, to even = up
    assert got[0, 1, 0, 2].item() == tiny                      # a denormal of T passes through
    assert got[0, 3, 1, 1].item() == 2 * tiny                  # 0 + 1.5 tiny: a tie among denormals, to even
    assert got[0, 2, 1, 0].item() == float("inf")              # big + big_bias overflows T
    assert torch.isnan(got[0, :, 1, 2]).all()
    assert same(out, want)


# ---- pool_max and its gradient ----------------------------------------------------------------------------------------------
POOL_NS = (1, 3, 4, 8, 16, 32, 64, 256, 257)
VALUES16 = [-3.0, -1.5, -1.0, -0.5, -0.25, -0.0, 0.0, 0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, 8.0]


def pool_rows(ns, kind):
    if kind == "one":
        return 1
    if kind == "seven":
        return 7
    vec = ns >= 8 and ns <= 256 and (ns & (ns - 1)) == 0
    return (256 // (ns // 8)) * 4 + 1 if vec else 17           # one row into the second workgroup


@functools.lru_cache(maxsize=None)
def pool_case(ns, kind, tname):
    dtype = TYPES[tname]
    rows = pool_rows(ns, kind)
    g = torch.Generator().manual_seed(100 + ns + rows)
    values = torch.tensor(VALUES16).to(dtype)
    x = values[torch.randint(0, 16, (rows, ns), generator=g)]
    if rows >= 7:
        x[1, ns // 2], x[1, ns - 1] = float("nan"), float("nan")
        x[2] = float("-inf")
        x[2, ns - 1] = float("inf")
        x[3] = 0.0
        x[3, 0::2] = -0.0                                      # -0 first: the tie keeps ITS bits
        x[4] = -0.0
        x[4, 0::2] = 0.0
        x[5] = float("-inf")
        x[6] = 2.0                                             # a whole row of ties
    want, arg = R.pool_max(x)
    grad = values[torch.randint(0, 16, (rows,), generator=g)]
    if rows >= 7:
        grad[3] = -0.0
    return x, want, arg, grad, R.pool_max_grad(grad, arg, ns)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("kind", ["one", "seven", "blocks"])
@pytest.mark.parametrize("ns", POOL_NS)
def test_pool_max_and_gradient(ns, kind, tname, off):
    dtype = TYPES[tname]
    x, want, want_arg, grad, want_gx = pool_case(ns, kind, tname)
    rows = x.shape[0]
    xd, out = at_offset(x, dtype, off), at_offset((rows,), dtype, off)
    arg = offset_alloc.output((rows,), torch.int32, 0)
    ext().pool_max_h_wrapper(rows, ns, xd, out, arg)
    out2 = at_offset((rows,), dtype, off)
    ext().pool_max_h_wrapper(rows, ns, xd, out2, None)          # arg=None: the inference form
    gd, gx = at_offset(grad, dtype, off), at_offset((rows, ns), dtype, off)
    ext().pool_max_grad_h_wrapper(rows, ns, gd, arg, gx)
    offset_alloc.check()
    assert same(out, want) and same(out2, want)
    assert torch.equal(arg.cpu(), want_arg)
    assert same(gx, want_gx)                                   # every element


# ---- three_interpolate ------------------------------------------------------------------------------------------------
TI_CASES = {            # (b, c, m, n)
    "staged": (2, 8, 64, 256),
    "c6": (2, 6, 64, 256),
    "smallest": (1, 4, 3, 5),
    "wide_staged": (1, 8, 4096, 1028),
}


@functools.lru_cache(maxsize=None)
def ti_case(name, tname):
    b, c, m, n = TI_CASES[name]
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(21 + len(name))
    points = (torch.randn((b, c, m), generator=g) * 2).to(dtype)
    idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32)
    idx[:, 0] = torch.tensor([0, m - 1, m - 1], dtype=torch.int32)      # both ends, a repeat
    idx[:, 1] = idx[:, 1, 0:1]                                           # one known point three times
    weight = torch.rand((b, n, 3), generator=g)
    weight = weight / weight.sum(dim=2, keepdim=True)
    weight[:, 2] = torch.tensor([1.0, 0.0, 0.0])                         # zero weights
    weight[:, 3] = 0.0
    return points, idx, weight, R.three_interpolate(points, idx, weight)


@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("tname", list(TYPES))
@pytest.mark.parametrize("name", list(TI_CASES))
def test_three_interpolate(name, tname, off):
    b, c, m, n = TI_CASES[name]
    dtype = TYPES[tname]
    points, idx, weight, want = ti_case(name, tname)
    pd, out = at_offset(points, dtype, off), at_offset((b, c, n), dtype, off)
    ext().three_interpolate_h_wrapper(b, c, m, n, pd, idx.to(DEV), weight.to(DEV), out)
    offset_alloc.check()
    assert same(out, want)


# ---- the operator layer: native ops through autograd, and the upcast route ---------------------------------------------------
def dyadic(shape, dtype, g, scale=4):
    """multiples of 1/scale in [-2, 2]: exact in both 16-bit types, and float32 sums of hundreds of them (and of their products
    with each other) are exact -- so a gradient that accumulates with atomics has ONE answer, whatever its order, and the
    restatement can pin its bits. The sums still need more mantissa bits than T has: the one rounding is exercised."""
    return (torch.randint(-2 * scale, 2 * scale + 1, shape, generator=g).float() / scale).to(dtype)


@pytest.mark.parametrize("tname", list(TYPES))
def test_ops_through_autograd(tname):
    """group_linear (native forward; grad_z by the upcast route, grad_w and grad_b float32), pool_max (native both ways),
    three_interpolate (native forward, upcast backward)"""
    from epnet_amd import pointnet2_utils as pu
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(31)
    b, c, n, m, ns = 2, 6, 40, 5, 4
    xyz = dyadic((b, n, 3), torch.float32, g, 8)
    new_xyz = xyz[:, :m].clone()
    z = dyadic((b, c, n), dtype, g)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    w, bias = dyadic((c, 3), torch.float32, g), dyadic((c,), torch.float32, g)
    zd = z.to(DEV).requires_grad_(True)
    wd, bd = w.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    hidden = pu.group_linear(xyz.to(DEV), new_xyz.to(DEV), zd, idx.to(DEV), wd, bd)
    assert hidden.dtype == dtype and same(hidden, R.group_linear(xyz, new_xyz, z, idx, w, bias))
    pooled = pu.pool_max(hidden)
    want_pool, want_arg = R.pool_max(hidden.detach().cpu().reshape(-1, ns))
    assert pooled.dtype == dtype and same(pooled.reshape(-1), want_pool)
    gp = dyadic((b, c, m, 1), dtype, g)
    pooled.backward(gp.to(DEV))
    g_hidden = R.pool_max_grad(gp.reshape(-1), want_arg, ns).reshape(b, c, m, ns)
    assert zd.grad.dtype == dtype and same(zd.grad, R.scatter_rows(g_hidden, idx, n))
    assert wd.grad.dtype == torch.float32 and same(wd.grad, R.group_linear_grad_w(g_hidden, xyz, new_xyz, idx))
    assert bd.grad.dtype == torch.float32 and same(bd.grad, g_hidden.float().sum(dim=(0, 2, 3)))

    mk, nu = 7, 12
    feats = dyadic((b, c, mk), dtype, g)
    tidx = torch.randint(0, mk, (b, nu, 3), generator=g, dtype=torch.int32)
    tw = dyadic((b, nu, 3), torch.float32, g).abs()
    fd = feats.to(DEV).requires_grad_(True)
    spread = pu.three_interpolate(fd, tidx.to(DEV), tw.to(DEV))
    assert spread.dtype == dtype and same(spread, R.three_interpolate(feats, tidx, tw))
    gs = dyadic((b, c, nu), dtype, g)
    spread.backward(gs.to(DEV))
    assert fd.grad.dtype == dtype and same(fd.grad, R.three_interpolate_grad(gs, tidx, tw, mk))


@pytest.mark.parametrize("tname", list(TYPES))
def test_upcast_route_gather_and_grouping(tname):
    from epnet_amd import pointnet2_utils as pu
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(41)
    b, c, n, m, ns = 2, 5, 33, 6, 3
    feats = torch.randn((b, c, n), generator=g).to(dtype)
    feats[0, 0, 0], feats[0, 0, 1] = -0.0, 2.0 ** -133 if dtype == torch.bfloat16 else 2.0 ** -24      # moves keep every bit
    idx1 = torch.randint(0, n, (b, m), generator=g, dtype=torch.int32)
    idx1[:, 0], idx1[:, 1] = 0, 1
    idx2 = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    idx2[:, 0, 0], idx2[:, 0, 1] = 0, 1
    f1 = feats.to(DEV).requires_grad_(True)
    out = pu.gather_operation(f1, idx1.to(DEV))
    assert out.dtype == dtype and same(out, R.gather(feats, idx1))
    go = dyadic((b, c, m), dtype, g)
    out.backward(go.to(DEV))
    assert f1.grad.dtype == dtype and same(f1.grad, R.scatter_rows(go, idx1, n))
    f2 = feats.to(DEV).requires_grad_(True)
    out = pu.grouping_operation(f2, idx2.to(DEV))
    assert out.dtype == dtype and same(out, R.grouping(feats, idx2))
    go = dyadic((b, c, m, ns), dtype, g)
    out.backward(go.to(DEV))
    assert f2.grad.dtype == dtype and same(f2.grad, R.scatter_rows(go, idx2, n))


@pytest.mark.parametrize("tname", list(TYPES))
def test_upcast_route_group_concat(tname):
    """with the coordinates in front: float32, torch.cat's promotion of (float32 xyz, T features); features alone: T"""
    from epnet_amd import pointnet2_utils as pu
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(43)
    b, c, n, m = 2, 4, 48, 6
    xyz = torch.randn((b, n, 3), generator=g)
    new_xyz = xyz[:, :m].clone()
    feats = torch.randn((b, c, n), generator=g).to(dtype)
    idxs = [torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32) for ns in (4, 8)]
    centred = [(torch.stack([xyz[k][i[k].long()] for k in range(b)]) - new_xyz[:, :, None, :]).permute(0, 3, 1, 2) for i in idxs]
    xd, nd = xyz.to(DEV), new_xyz.to(DEV)
    fd = feats.to(DEV).requires_grad_(True)
    grouper = pu.QueryAndGroup(1.0, 4, use_xyz=True)
    both = grouper(xd, nd, fd, idx=idxs[0].to(DEV))
    assert both.dtype == torch.float32
    assert same(both, torch.cat([centred[0], R.grouping(feats, idxs[0]).float()], dim=1))
    go = dyadic(tuple(both.shape), torch.float32, g)
    both.backward(go.to(DEV))
    assert fd.grad.dtype == dtype and same(fd.grad, R.scatter_rows(go[:, 3:].to(dtype), idxs[0], n))
    alone = pu.QueryAndGroup(1.0, 4, use_xyz=False)(xd, nd, feats.to(DEV), idx=idxs[0].to(DEV))
    assert alone.dtype == dtype and same(alone, R.grouping(feats, idxs[0]))
    multi = pu.group_concat_multi(xd, nd, feats.to(DEV), [i.to(DEV) for i in idxs], use_xyz=True)
    for k in range(2):
        assert multi[k].dtype == torch.float32
        assert same(multi[k], torch.cat([centred[k], R.grouping(feats, idxs[k]).float()], dim=1))
    multi = pu.group_concat_multi(xd, nd, feats.to(DEV), [i.to(DEV) for i in idxs], use_xyz=False)
    for k in range(2):
        assert multi[k].dtype == dtype and same(multi[k], R.grouping(feats, idxs[k]))


@pytest.mark.parametrize("tname", list(TYPES))
def test_upcast_route_feature_gather(tname):
    """the float32 sampler on the upcast map, rounded once -- forwards at arbitrary pixels, backwards at pixel centres with
    dyadic gradients (one answer whatever the order of the atomics)"""
    from epnet_amd.li_fusion import Feature_Gather
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(47)
    b, c, h, w, n = 2, 3, 5, 9, 20
    fmap = torch.randn((b, c, h, w), generator=g).to(dtype)
    xy = (torch.rand((b, n, 2), generator=g) * 2 - 1).to(DEV)
    got = Feature_Gather(fmap.to(DEV), xy)
    want = Feature_Gather(fmap.float().to(DEV), xy).cpu().to(dtype)
    assert got.dtype == dtype and same(got, want)
    px = torch.stack([torch.randint(0, w, (b, n), generator=g).float() / (w - 1), torch.randint(0, h, (b, n), generator=g).float() / (h - 1)], dim=2)
    centres = (px * 2 - 1).to(DEV)                              # exact pixel centres under align_corners=True: weights 1 and 0
    fd = fmap.to(DEV).requires_grad_(True)
    out = Feature_Gather(fd, centres)
    go = dyadic((b, c, n), dtype, g)
    out.backward(go.to(DEV))
    f32 = fmap.float().to(DEV).requires_grad_(True)
    Feature_Gather(f32, centres).backward(go.float().to(DEV))
    assert fd.grad.dtype == dtype and same(fd.grad, f32.grad.cpu().to(dtype))


@pytest.mark.parametrize("tname", list(TYPES))
def test_deterministic_mode_takes_the_det_twins(tname):
    """arbitrary values: under torch's deterministic mode the gradient is the `_det` entry point on the upcast grad_out, rounded
    once -- the float32 op in the same mode is that entry point"""
    from epnet_amd import pointnet2_utils as pu
    dtype = TYPES[tname]
    g = torch.Generator().manual_seed(53)
    b, c, n, m, ns = 2, 6, 40, 8, 4
    xyz = torch.randn((b, n, 3), generator=g).to(DEV)
    new_xyz = xyz[:, :m].contiguous()
    z = torch.randn((b, c, n), generator=g).to(dtype)
    idx = torch.randint(0, 6, (b, m, ns), generator=g, dtype=torch.int32).to(DEV)       # many repeats
    w, bias = torch.randn((c, 3), generator=g).to(DEV), torch.randn((c,), generator=g).to(DEV)
    go = torch.randn((b, c, m, ns), generator=g).to(dtype)
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        grads = []
        for t in (dtype, torch.float32):
            zd, wd = z.to(t).to(DEV).requires_grad_(True), w.clone().requires_grad_(True)
            pu.group_linear(xyz, new_xyz, zd, idx, wd, bias).backward(go.to(t).to(DEV))
            fd = z.to(t).to(DEV).requires_grad_(True)
            pu.grouping_operation(fd, idx).backward(go.to(t).to(DEV))
            grads.append((zd.grad, wd.grad, fd.grad))
    finally:
        torch.use_deterministic_algorithms(was)
    (gz16, gw16, gf16), (gz32, gw32, gf32) = grads
    assert gz16.dtype == dtype and same(gz16, gz32.to(dtype))
    assert gw16.dtype == torch.float32 and same(gw16, gw32)
    assert gf16.dtype == dtype and same(gf16, gf32.to(dtype))


@pytest.mark.parametrize("tname", list(TYPES))
def test_graph_capture_and_replay(tname):
    """group_linear then pool_max captured into a HIP graph, replayed on new bits of z: equals the eager result"""
    dtype = TYPES[tname]
    b, c, n, m, ns = 2, 8, 256, 16, 16
    g = torch.Generator().manual_seed(61)
    xyz = torch.randn((b, n, 3), generator=g)
    new_xyz = xyz[:, :m].clone()
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    w, bias = torch.randn((c, 3), generator=g), torch.randn((c,), generator=g)
    z1, z2 = (torch.randn((b, c, n), generator=g).to(dtype) for _ in range(2))
    xd, nd, idd, wd, bd = xyz.to(DEV), new_xyz.to(DEV), idx.to(DEV), w.to(DEV), bias.to(DEV)
    zs = z1.to(DEV)
    hidden = torch.empty((b, c, m, ns), dtype=dtype, device=DEV)
    pooled = torch.empty((b, c, m), dtype=dtype, device=DEV)
    arg = torch.empty((b, c, m), dtype=torch.int32, device=DEV)
    e = ext()

    def run():
        e.group_linear_h_wrapper(b, c, n, m, ns, xd, nd, zs, idd, wd, bd, hidden)
        e.pool_max_h_wrapper(b * c * m, ns, hidden, pooled, arg)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    zs.copy_(z2.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = (hidden.clone(), pooled.clone(), arg.clone())
    run()
    torch.cuda.synchronize()
    assert same(replayed[0], hidden) and same(replayed[1], pooled) and torch.equal(replayed[2], arg)
    want = R.group_linear(xyz, new_xyz, z2, idx, w, bias)
    assert same(replayed[0], want) and same(replayed[1].reshape(-1), R.pool_max(want.reshape(-1, ns))[0])


def test_float64_still_raises():
    from epnet_amd import pointnet2_utils as pu
    g = torch.Generator().manual_seed(71)
    xyz = torch.randn((1, 8, 3), generator=g).to(DEV)
    idx = torch.zeros((1, 2, 4), dtype=torch.int32, device=DEV)
    z = torch.randn((1, 2, 8), generator=g).double().to(DEV)
    with pytest.raises(RuntimeError, match="dtype"):
        pu.group_linear(xyz, xyz[:, :2].contiguous(), z, idx, torch.zeros((2, 3), device=DEV))
    with pytest.raises(RuntimeError, match="dtype"):
        pu.pool_max(z)
    with pytest.raises(RuntimeError, match="dtype"):
        pu.three_interpolate(z, torch.zeros((1, 5, 3), dtype=torch.int32, device=DEV), torch.ones((1, 5, 3), device=DEV))
    with pytest.raises(RuntimeError, match="dtype"):
        pu.grouping_operation(z, idx)
    with pytest.raises(RuntimeError, match="dtype"):      # 16-bit weights are not feature rows
        pu.group_linear(xyz, xyz[:, :2].contiguous(), z.bfloat16(), idx, torch.zeros((2, 3), device=DEV, dtype=torch.bfloat16))


@pytest.mark.parametrize("shape", [(2, 8, 256, 64, 16), (2, 3, 64, 5, 3)])       # the float32 staged and scalar kernels
def test_float32_bits_unchanged(shape):
    """float32 inputs take the float32 entry points and give the documented expression's bits, as before"""
    from epnet_amd import pointnet2_utils as pu
    b, c, n, m, ns = shape
    g = torch.Generator().manual_seed(73)
    xyz = torch.randn((b, n, 3), generator=g)
    new_xyz = xyz[:, :m].clone()
    z = torch.randn((b, c, n), generator=g)
    idx = torch.randint(0, n, (b, m, ns), generator=g, dtype=torch.int32)
    w, bias = torch.randn((c, 3), generator=g), torch.randn((c,), generator=g)
    hidden = pu.group_linear(xyz.to(DEV), new_xyz.to(DEV), z.to(DEV), idx.to(DEV), w.to(DEV), bias.to(DEV))
    want = R.group_linear(xyz, new_xyz, z, idx, w, bias)
    assert hidden.dtype == torch.float32 and same(hidden, want)
    pooled = pu.pool_max(hidden)
    assert pooled.dtype == torch.float32 and same(pooled.reshape(-1), R.pool_max(want.reshape(-1, ns))[0])
    tidx = torch.randint(0, n, (b, m * ns, 3), generator=g, dtype=torch.int32)
    tw = torch.rand((b, m * ns, 3), generator=g)
    spread = pu.three_interpolate(z.to(DEV), tidx.to(DEV), tw.to(DEV))
    assert spread.dtype == torch.float32 and same(spread, R.three_interpolate(z, tidx, tw))
