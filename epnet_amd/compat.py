"""Import-path compatibility with the reference tree.

The reference's Python surface does bare top-level imports of its three extensions
(``import pointnet2_cuda as pointnet2`` pointnet2_utils.py:7, ``import iou3d_cuda`` iou3d_utils.py:2,
``import roipool3d_cuda`` roipool3d_utils.py:2) and its model code imports the surface as
``pointnet2_lib.pointnet2.pointnet2_modules`` (lib/net/pointnet2_msg.py:4),
``pointnet2_lib.pointnet2.pytorch_utils`` (lib/net/rpn.py:5), ``lib.utils.iou3d.iou3d_utils``
(lib/rpn/proposal_layer.py:6), ``lib.utils.roipool3d.roipool3d_utils`` (lib/net/rcnn_net.py:4).

``install_extensions()`` makes the three extension names resolve to this package's stand-ins, so an
unmodified reference checkout runs on MI355X (its own Python surface on top of our C ABI).
``install_surface()`` additionally serves this package's surface modules under the reference's
package paths for callers that do not have the reference tree on ``sys.path`` at all.
``install_evaluator()`` serves the AP evaluator under ``tools.kitti_object_eval_python`` (tools/eval_rcnn.py:11), whose
reference modules need numba and a CUDA device.
"""
import importlib
import sys
import types

_EXT = ("pointnet2_cuda", "iou3d_cuda", "roipool3d_cuda")
_SURFACE = {
    "pointnet2_lib.pointnet2.pointnet2_utils": "pointnet2_utils",
    "pointnet2_lib.pointnet2.pointnet2_modules": "pointnet2_modules",
    "pointnet2_lib.pointnet2.pytorch_utils": "pytorch_utils",
    "lib.utils.iou3d.iou3d_utils": "iou3d_utils",
    "lib.utils.roipool3d.roipool3d_utils": "roipool3d_utils",
}


# the "next" rows of SURVEY.md 8(f): the callers either side of the NMS / IoU / pooling ops
_CALLERS = {
    "lib.rpn.proposal_layer": "proposal_layer",                  # lib/net/rpn.py:4 imports ProposalLayer from here
    "lib.rpn.proposal_target_layer": "proposal_target_layer",    # lib/net/rcnn_net.py:5 imports ProposalTargetLayer from here
}


def install_extensions():
    for name in _EXT:
        sys.modules[name] = importlib.import_module("epnet_amd." + name)


def _ensure_package(dotted):
    """create empty namespace packages for the parents of `dotted` unless real ones are importable"""
    parts = dotted.split(".")[:-1]
    for i in range(1, len(parts) + 1):
        pkg = ".".join(parts[:i])
        if pkg in sys.modules:
            continue
        try:
            importlib.import_module(pkg)
        except Exception:
            mod = types.ModuleType(pkg)
            mod.__path__ = []
            sys.modules[pkg] = mod
            if i > 1:
                setattr(sys.modules[".".join(parts[:i - 1])], parts[i - 1], mod)


def install_surface(include_kitti_utils=False):
    install_extensions()
    table = dict(_SURFACE)
    if include_kitti_utils:  # only the 3 helpers exist here; leave the real module alone if present
        table["lib.utils.kitti_utils"] = "kitti_utils"
    for dotted, local in table.items():
        _ensure_package(dotted)
        mod = importlib.import_module("epnet_amd." + local)
        sys.modules[dotted] = mod
        parent, leaf = dotted.rsplit(".", 1)
        setattr(sys.modules[parent], leaf, mod)


def install_callers(sync_free=False, fused_head=False):
    """serve this package's ProposalLayer / ProposalTargetLayer under the reference's module paths, so that
    lib/net/rpn.py and lib/net/rcnn_net.py construct them unchanged; both read the reference's ``lib.config.cfg`` when
    that module is loaded (same attribute names), their own yaml-valued defaults otherwise. The default target layer is the
    draw-for-draw restatement of the reference's host random streams; sync_free=True serves
    ``rcnn_target_layer.RCNNTargetLayer`` (same distributions, device tables, no host synchronisation) under the reference's
    class name instead. fused_head=True serves a ProposalLayer whose forward is one ``epnet_rpn_handover`` call (decoding, score
    order and proposals; rpn_handover.py) under the reference's class name.

    The optimiser is not served under a module path: tools/train_rcnn.py builds it inline. ``create_optimizer(model)`` +
    ``create_scheduler(optimizer, total_steps, last_epoch)`` with TRAIN.OPTIMIZER adam_onecycle map onto
    ``fused_adam_onecycle(model, cfg, total_steps)`` below, and train_utils.py:126-136 onto its ``step()``"""
    install_extensions()
    for dotted, local in _CALLERS.items():
        _ensure_package(dotted)
        mod = importlib.import_module("epnet_amd." + local)
        if sync_free and local == "proposal_target_layer":
            fused = importlib.import_module("epnet_amd.rcnn_target_layer")
            mod = types.ModuleType(dotted)
            mod.__dict__.update({k: v for k, v in vars(fused).items() if not k.startswith("__")})
            mod.ProposalTargetLayer = fused.RCNNTargetLayer
        if fused_head and local == "proposal_layer":
            stock = mod

            class ProposalLayer(stock.ProposalLayer):
                def __init__(self, mode='TRAIN', cfg=None):
                    super().__init__(mode, cfg, fused_head=True)

            mod = types.ModuleType(dotted)
            mod.__dict__.update({k: v for k, v in vars(stock).items() if not k.startswith("__")})
            mod.ProposalLayer = ProposalLayer
        sys.modules[dotted] = mod
        parent, leaf = dotted.rsplit(".", 1)
        setattr(sys.modules[parent], leaf, mod)


def fused_adam_onecycle(model, cfg, total_steps, **kwargs):
    """``epnet_amd.optim.FusedAdamOneCycle`` from the reference's ``cfg.TRAIN`` (LR, MOMS, DIV_FACTOR, PCT_START, WEIGHT_DECAY,
    GRAD_NORM_CLIP; Adam's beta2 = 0.99 is tools/train_rcnn.py:110's). It takes the place of create_optimizer + create_scheduler
    (tools/train_rcnn.py:98-146) for TRAIN.OPTIMIZER adam_onecycle, and its ``step()`` the place of clip_grad_norm_ +
    lr_scheduler.step(it) + optimizer.step() in the trainer (train_utils.py:126-136, :186-187). Freeze the RPN (RPN.FIXED)
    AFTER this call, as the reference does: the state dict then keeps the reference's parameter order."""
    from . import optim
    t = cfg.TRAIN
    return optim.FusedAdamOneCycle(model, total_steps, lr_max=t.LR, moms=tuple(t.MOMS), div_factor=t.DIV_FACTOR, pct_start=t.PCT_START,
                                   wd=t.WEIGHT_DECAY, grad_norm_clip=t.GRAD_NORM_CLIP, **kwargs)


_EVALUATOR = "tools.kitti_object_eval_python"


def install_evaluator():
    """serve ``epnet_amd.kitti_eval`` as ``tools.kitti_object_eval_python.evaluate`` / ``.eval`` / ``.kitti_common`` and its
    ``rotate_iou_gpu_eval(boxes, query_boxes, criterion)`` as ``.rotate_iou``, so that ``from
    tools.kitti_object_eval_python.evaluate import evaluate`` (tools/eval_rcnn.py:11) resolves without numba"""
    mod = importlib.import_module("epnet_amd.kitti_eval")
    rot = types.ModuleType(_EVALUATOR + ".rotate_iou")
    rot.rotate_iou_gpu_eval = mod.rotate_iou_gpu_eval
    for leaf, served in (("evaluate", mod), ("eval", mod), ("kitti_common", mod), ("rotate_iou", rot)):
        dotted = _EVALUATOR + "." + leaf
        _ensure_package(dotted)
        sys.modules[dotted] = served
        setattr(sys.modules[_EVALUATOR], leaf, served)
