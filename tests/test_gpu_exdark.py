"""GPU: the stage-2 ExDark evaluation (millieye_amd.module2.test_mixed, module2_mixed/test_mixed.py) and its batched input
producer (me_image_batch_pad_resize_flip_u8_f32) against the per-frame kernel and the REAL reference's outputs on the small
ExDark tree (tests/golden/exdark_eval_small.npz, tests/golden/make_golden_exdark.py)."""
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden_exdark import EXDARK, NAME, RUN, STORE_STRIDE, fill_detector_, weighted_sum

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _frames(tag, shapes):
    from millieye_amd import synth
    return [torch.from_numpy(synth.uniform(f"{tag}/{i}", (h, w, 3), 0, 256).astype(np.uint8)) for i, (h, w) in enumerate(shapes)]


def test_batched_producer_equals_per_frame_kernel(hip_lib):
    """Ragged batches (landscape, portrait, square, odd / even differences), with and without flips, S < P, S > P, S == P
    and S % 4 != 0 (the one-pixel-per-thread path): every frame bit-identical to me_image_pad_resize_flip_u8_f32."""
    from millieye_amd.utils.datasets import StagedImages, StagedRaggedImages
    shapes = [(37, 91), (91, 37), (64, 64), (120, 75), (300, 420), (33, 32), (1, 5), (450, 800)]
    frames = _frames("exdark/batch", shapes)
    flips = [False, True, True, False, True, False, True, True]
    for size in (64, 416, 33, 450, 96):
        got = StagedRaggedImages(frames, size, flips=flips).to("cuda")
        ref = StagedImages(frames, size, flips=flips).to("cuda")
        torch.cuda.synchronize()
        assert got.shape == (len(frames), 3, size, size)
        for i in range(len(frames)):
            assert torch.equal(got[i], ref[i]), (size, i, shapes[i], float((got[i] - ref[i]).abs().max()))
    one = StagedRaggedImages(frames[:1], 64, flips=[True]).type(torch.cuda.FloatTensor)
    assert torch.equal(one[0], StagedImages(frames[:1], 64, flips=[True]).to("cuda")[0])


def test_exdark_batches_match_reference(hip_lib):
    """ExDarkDataset batches through the unchanged reference call ``imgs.type(torch.cuda.FloatTensor)``: images equal to the
    reference's (uint8 codes of k / 255 and the position-weighted checksum), targets exact."""
    from millieye_amd.module2.datasets import ExDarkDataset
    g = np.load(os.path.join(GOLD, NAME + ".npz"))
    for size in EXDARK["sizes"]:
        ds = ExDarkDataset("test", coco_detector=False, img_size=size, augment=False, multiscale=False, root=RUN)
        loader = torch.utils.data.DataLoader(ds, batch_size=EXDARK["batch"], shuffle=False, num_workers=0,
                                             collate_fn=ds.collate_fn)
        for b, (_paths, imgs, targets) in enumerate(loader):
            x = imgs.type(torch.cuda.FloatTensor)
            assert x.is_cuda and x.shape[1:] == (3, size, size)
            host = x.cpu()
            codes = torch.round(host * 255).to(torch.uint8)
            assert torch.equal(codes.float() / 255, host)   # (on the host: the reference's division)
            st = STORE_STRIDE[size]
            assert np.array_equal(codes.numpy()[:, :, ::st, ::st], g[f"b{size}/{b}/codes"]), (size, b)
            assert np.array_equal(weighted_sum(host), g[f"b{size}/{b}/imgs_wsum"]), (size, b)
            assert np.array_equal(targets.numpy(), g[f"b{size}/{b}/targets"]), (size, b)


def _model(dtype=None):
    from millieye_amd.yolov3.models import Darknet
    from tests.parity_helpers import cfg_path
    model = fill_detector_(Darknet(cfg_path(EXDARK["cfg"]))).cuda().eval()
    if dtype is not None:
        model.compute_dtype = dtype
    return model


def _evaluate(model, size):
    from millieye_amd.module2.test_mixed import evaluate
    return evaluate(model, mode="test", iou_thres=EXDARK["iou"], conf_thres=EXDARK["conf"], nms_thres=EXDARK["nms"],
                    img_size=size, batch_size=EXDARK["batch"], root=RUN, num_workers=0)


def test_evaluate_matches_reference(hip_lib):
    """``test_mixed.evaluate`` end to end (ExDarkDataset, the detector with the NMS candidate decode, NMS, the pre-NMS counts,
    the device batch statistics, module 2's ap_per_class) against the reference's evaluate: box_stat equal, classes equal,
    metrics and the P-R curve within 1e-9."""
    g = np.load(os.path.join(GOLD, NAME + ".npz"))
    model = _model()
    for size in EXDARK["sizes"]:
        precision, recall, AP, f1, ap_class, box_stat, pr_curve = _evaluate(model, size)
        k = f"eval{size}/"
        assert list(box_stat["before"]) == list(g[k + "before"]), size
        assert list(box_stat["after"]) == list(g[k + "after"]), size
        assert list(ap_class) == list(g[k + "ap_class"])
        for name, got in (("precision", precision), ("recall", recall), ("AP", AP), ("f1", f1)):
            assert np.allclose(got, g[k + name], rtol=0, atol=1e-9), (size, name, got, g[k + name])
        assert len(pr_curve) == 3
        for j in (0, 1):
            assert np.allclose(pr_curve[j], g[k + f"pr_curve{j}"], rtol=0, atol=1e-9), (size, j)
        assert np.allclose(pr_curve[2], g[k + "pr_curve2"], rtol=0, atol=1e-3), size
    assert AP[0] > 0   # 416: the frames and the targets are on the same scale


@pytest.mark.parametrize("dtype,ap_tol", [("bf16", 0.03), ("f16", 0.03)])
def test_evaluate_in_16bit_storage_modes(hip_lib, dtype, ap_tol):
    """The detector in a 16-bit storage mode against the reference's fp32 numbers: same classes, AP / precision / recall
    within ``ap_tol`` absolute.  3 points for both modes: every class of this fixture has only a handful of targets, so one
    swap of two neighbouring detections in the confidence order moves its AP by more than a point (IEEE half: 1.2 points on
    one class; the stage-3 fixture holds half to 1 point)."""
    g = np.load(os.path.join(GOLD, NAME + ".npz"))
    k = "eval416/"
    precision, recall, AP, f1, ap_class, box_stat, _pr = _evaluate(_model(dtype), 416)
    assert list(ap_class) == list(g[k + "ap_class"])
    for name, got in (("precision", precision), ("recall", recall), ("AP", AP)):
        assert np.all(np.abs(np.asarray(got) - g[k + name]) <= ap_tol), (dtype, name, got, g[k + name])
    print(f"{dtype}: AP {np.asarray(AP)} (reference fp32 {g[k + 'AP']}), before {box_stat['before']}")
