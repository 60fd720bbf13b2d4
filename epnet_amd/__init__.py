"""epnet_amd -- MI355X-native (gfx950) point-cloud geometry operators of EPNet / PointRCNN.

The package holds only what the hot path needs:

* ``csrc/``          hand-written HIP kernels + the C ABI (``include/epnet_ops.h``) -> ``lib/libepnet_hip.so``
* ``_lib``           ctypes loader of that library (fails loudly when it is missing)
* ``pointnet2_cuda``, ``iou3d_cuda``, ``roipool3d_cuda``
                     drop-in stand-ins for the reference's three extension modules (same function
                     names and positional signatures), backed by the C ABI
* ``pointnet2_utils``, ``pointnet2_modules``, ``pytorch_utils``, ``iou3d_utils``,
  ``roipool3d_utils``, ``kitti_utils``
                     the reference's Python operator surface, re-provided with identical names
* ``loss_cuda``, ``loss_utils``
                     the training losses (``lib/net/train_functions.py``'s two closures) as one fused call each, forward
                     and backward, with no host synchronisation
* ``rpn_target_cuda``, ``rpn_target_layer``
                     the RPN training targets (the loader's augmentation and per-point labels) of a whole batch as one
                     launch, with no host synchronisation
* ``compat``         registers all of the above under the import paths the reference's callers use
* ``synth``, ``sa_stack``  synthetic KITTI-shaped inputs and the SA/FP op-stack driver used by bench.py

There is no CPU fallback: device ops raise if the HIP library is absent or a tensor is not on a GPU.
"""
__version__ = "0.1.0"
