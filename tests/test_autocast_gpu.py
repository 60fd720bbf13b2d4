"""The SA / FP levels under torch.autocast: the two-stream backbone and an RCNN-stage SA level run forward and backward in
bfloat16, forward in float16, the RPN loss takes bfloat16 head outputs, and the whole two-stage step runs with either target
layer. What is asserted is the plumbing -- the types
between the levels, float32 parameter gradients, finite values. No model-level numeric bound: the dense layers are stock and
the operators are pinned bit for bit in tests/test_rows16_gpu.py. Convergence under bfloat16 is not tested."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _small_backbone():
    from epnet_amd.rpn_backbone import BackboneConfig, Pointnet2MSG
    torch.manual_seed(0)
    return Pointnet2MSG(input_channels=0, config=BackboneConfig(image_size=[64.0, 32.0]), scale=16).to(DEV)


def _scene(g, b=2, n=1024):
    pts = torch.rand((b, n, 3), generator=g) * torch.tensor([8.0, 2.0, 8.0])
    image = torch.randn((b, 3, 32, 64), generator=g)
    xy = torch.rand((b, n, 2), generator=g) * torch.tensor([63.0, 31.0])
    return pts.to(DEV), image.to(DEV), xy.to(DEV)


def _level_dtypes(model):
    seen = []
    hooks = [sa.register_forward_hook(lambda mod, args, out: seen.append(out[1].dtype)) for sa in model.SA_modules]
    hooks += [fp.register_forward_hook(lambda mod, args, out: seen.append(out.dtype)) for fp in model.FP_modules]
    return seen, hooks


def test_backbone_trains_under_bf16_autocast():
    model = _small_backbone().train()
    pts, image, xy = _scene(torch.Generator().manual_seed(1))
    image.requires_grad_(True)
    seen, hooks = _level_dtypes(model)
    with torch.autocast("cuda", torch.bfloat16):
        xyz, feats = model(pts, image, xy)
    for h in hooks:
        h.remove()
    assert len(seen) == 8 and all(d == torch.bfloat16 for d in seen), seen      # four SA and four FP levels
    assert xyz.dtype == torch.float32 and feats.dtype == torch.bfloat16 and feats.shape == (2, 128, 1024)
    assert bool(torch.isfinite(feats.float()).all())
    feats.float().square().mean().backward()
    assert image.grad is not None and bool(torch.isfinite(image.grad).all())
    grads = [(name, p.grad) for name, p in model.named_parameters()]
    assert all(gr is not None and gr.dtype == torch.float32 for _, gr in grads), [n for n, gr in grads if gr is None]
    assert all(bool(torch.isfinite(gr).all()) for _, gr in grads)
    assert any(float(gr.abs().max()) > 0 for name, gr in grads if name.startswith("SA_modules.0"))


def test_backbone_forward_under_fp16_autocast():
    model = _small_backbone().eval()
    pts, image, xy = _scene(torch.Generator().manual_seed(2))
    seen, hooks = _level_dtypes(model)
    with torch.no_grad(), torch.autocast("cuda", torch.float16):
        _, feats = model(pts, image, xy)
    for h in hooks:
        h.remove()
    assert all(d == torch.float16 for d in seen), seen
    assert feats.dtype == torch.float16 and bool(torch.isfinite(feats.float()).all())


@pytest.mark.parametrize("mode", ["bf16_train", "fp16_infer"])
def test_rcnn_stage_sa_level(mode):
    """8 pooled clouds of 512 points, each a shorter cloud repeated cyclically (what ROI pooling hands over): features present,
    so the level folds its first layer -- matmul, group_linear, the rest of the MLP, pool_max, all in the autocast type"""
    from epnet_amd.pointnet2_modules import PointnetSAModule
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(3)
    sa = PointnetSAModule(npoint=128, radius=0.2, nsample=64, mlp=[128, 128, 128, 128], use_xyz=True, bn=True).to(DEV)
    unique = [37, 100, 200, 256, 300, 411, 511, 512]
    clouds, feats = [], []
    for u in unique:
        p, f = torch.rand((u, 3), generator=g), torch.randn((128, u), generator=g)
        reps = math.ceil(512 / u)
        clouds.append(p.repeat(reps, 1)[:512])
        feats.append(f.repeat(1, reps)[:, :512])
    xyz, features = torch.stack(clouds).to(DEV), torch.stack(feats).to(DEV)
    if mode == "bf16_train":
        sa.train()
        features.requires_grad_(True)
        with torch.autocast("cuda", torch.bfloat16):
            new_xyz, out, _ = sa(xyz, features)
        assert out.dtype == torch.bfloat16 and out.shape == (8, 128, 128) and new_xyz.dtype == torch.float32
        out.float().sum().backward()
        assert features.grad.dtype == torch.float32 and bool(torch.isfinite(features.grad).all())
        for p in sa.parameters():
            assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all())
    else:
        sa.eval()
        with torch.no_grad(), torch.autocast("cuda", torch.float16):
            _, out, _ = sa(xyz, features)
        assert out.dtype == torch.float16
    assert bool(torch.isfinite(out.float()).all())


def test_rpn_loss_on_bf16_heads():
    from epnet_amd import loss_utils
    cfg = loss_utils.default_cfg()
    g = torch.Generator().manual_seed(5)
    b, n = 2, 512
    channels = int(cfg.RPN.LOC_SCOPE / cfg.RPN.LOC_BIN_SIZE) * 2 * 4 + 1 + 2 * cfg.RPN.NUM_HEAD_BIN + 3
    cls = torch.randn((b, n, 1), generator=g).to(DEV).bfloat16().requires_grad_(True)
    reg = torch.randn((b, n, channels), generator=g).to(DEV).bfloat16().requires_grad_(True)
    u = torch.rand((b, n), generator=g)
    label = torch.where(u < 0.1, 1, torch.where(u > 0.9, -1, 0)).long().to(DEV)
    box = torch.cat([torch.rand((b, n, 3), generator=g) * 4 - 2, torch.rand((b, n, 3), generator=g) + 1.0,
                     torch.rand((b, n, 1), generator=g) * 6 - 3], dim=2).to(DEV)
    out = loss_utils.rpn_loss(cls, reg, label, box, cfg)
    assert out.loss.dtype == torch.float32 and bool(torch.isfinite(out.loss))
    out.loss.backward()
    assert cls.grad.dtype == torch.bfloat16 and reg.grad.dtype == torch.bfloat16     # cast back to the heads' type
    assert bool(torch.isfinite(cls.grad.float()).all()) and bool(torch.isfinite(reg.grad.float()).all())
    assert float(cls.grad.float().abs().max()) > 0


@pytest.mark.parametrize("targets", ["host", "fused"])
def test_two_stage_step_under_bf16_autocast(targets):
    """the whole rcnn_online step at a small scale: bfloat16 backbone features and head outputs pass the proposal layer, either
    target layer and the real losses -- whose box geometry stays float32 inside the autocast region -- and every parameter gets a
    finite float32 gradient"""
    import numpy as np
    import bench_step
    from epnet_amd import proposal_layer as pl, proposal_target_layer as ptl, rcnn_target_layer as rtl
    torch.manual_seed(0)
    np.random.seed(0)
    model = bench_step.build_model(scale=8, loss="reference").to(DEV)
    layers = (pl.ProposalLayer("TRAIN", fused_head=targets == "fused").to(DEV), ptl.ProposalTargetLayer() if targets == "host" else rtl.RCNNTargetLayer())
    xyz, gts = bench_step.synthetic_batch(2, 2048, 7, DEV)
    model.rpn_labels = bench_step.rpn_labels(xyz, gts)
    with torch.autocast("cuda", torch.bfloat16):
        loss, out = bench_step.run_step(model, layers, xyz, gts)
    assert out["rpn_cls"].dtype == torch.bfloat16 and out["rcnn_reg"].dtype == torch.bfloat16
    assert out["rois"].dtype == torch.float32 and out["target"]["sampled_pts"].dtype == torch.float32
    assert out["target"]["pts_feature"].dtype == torch.float32
    assert loss.dtype == torch.float32 and bool(torch.isfinite(loss))
    loss.backward()
    for name, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == torch.float32 and bool(torch.isfinite(p.grad).all()), name
