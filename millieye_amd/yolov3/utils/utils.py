"""The vendored PyTorch-YOLOv3 tree's ``non_max_suppression`` (reference ``yolov3/utils/utils.py:231-293``) on the GPU.

This module holds **only this function**: the rest of the reference's ``yolov3/utils/utils.py`` (metrics, ``build_targets``,
box helpers) is the same code as ``utils/utils.py`` and lives in :mod:`millieye_amd.utils.utils`.
"""
from ...utils.utils import python_nms

__all__ = ["non_max_suppression"]


def non_max_suppression(prediction, conf_thres=0.4, nms_thres=0.5):
    """Confidence filter + Python NMS with box merging (reference ``yolov3/utils/utils.py:231-293``).

    ``prediction`` ``[N,R,5+C]`` with (cx,cy,w,h,obj,cls...) rows; its first four columns are converted to xyxy **in
    place**.  Candidates: ``obj >= conf_thres``, ranked by ``obj * cls_conf`` (ties: lower row first).  The best alive box is
    kept and removes every alive box of the same ``cls_pred`` whose +1-pixel IoU with it is ``>= nms_thres``; its own box
    becomes the objectness-weighted mean of the boxes it removes, itself included (summed in float64 in a fixed order: two
    calls give the same bits).  Returns a list of ``[k,7]`` tensors (x1,y1,x2,y2,obj,cls_conf,cls_pred) on
    ``prediction.device`` or ``None`` for images without candidates.

    One departure from the reference: a kept box always removes itself.  The reference loops forever when the top box
    fails its own test (NaN coordinates, ``w + 1 <= 0``, ``nms_thres > 1``); here such a box is kept once as a cluster of one.

    The work runs in the ``me_nms_python_f32`` HIP kernels (``csrc/nms_py.hip``)."""
    return python_nms(prediction, conf_thres, nms_thres, score_mode=1, inclusive=True, merge=True)
