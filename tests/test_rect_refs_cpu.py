"""tests/rect_refs.py (the float64 restatements the rectangular GPU tests compare with) pinned to the oracle where the oracle can
run: square frames.  tiny-12 at 64 and 96, at the bar the oracle itself is pinned to its fixtures with (1e-5)."""
import pytest
import torch

from millieye_amd import cfgs, synth
from tests import parity_helpers as ph
from tests import rect_refs

TOL = 1e-5
NAME = "yolov3-tiny-12"


@pytest.mark.parametrize("n,s", [(2, 64), (1, 96)])
def test_darknet_forward_rect_equals_the_oracle_on_square_frames(n, s):
    from oracle import darknet_ref
    from millieye_amd.engine import pick_tap_module
    model = ph.make_darknet(NAME)
    x = ph.frames(f"rectref/{n}/{s}", n, s)
    tap = pick_tap_module(model.module_defs)
    ref_fm, ref_rows = darknet_ref.darknet_forward(ph.cfg_text(NAME), model.state_dict(), x, tap_module=tap)
    fm, rows, frac = rect_refs.darknet_forward_rect(model, x, tap, return_frac=True)
    assert fm.dtype == torch.float64 and rows.dtype == torch.float64
    assert tuple(fm.shape) == (n, 256, s // 16, s // 16)
    ph.assert_close(fm, ref_fm, TOL, "featuremap")
    ph.assert_close(rows, ref_rows, TOL, "rows")
    # the row order the cell test relies on: cell = floor(x / stride) wherever the fraction is not at a border
    stride, gx, gy = rect_refs.row_cells(model, s, s)
    keep = ~rect_refs.edge_rows(frac)
    assert torch.equal(torch.floor(rows[..., 0] / stride)[keep], gx.expand(n, -1)[keep].double())
    assert torch.equal(torch.floor(rows[..., 1] / stride)[keep], gy.expand(n, -1)[keep].double())


def test_rect_decode_is_the_square_decode_on_a_crop():
    """Cell (gy, gx) of a crop decodes to what it decodes to in the whole map (same stride): the rule is per cell."""
    from oracle import darknet_ref
    anchors, nc = [(10, 14), (23, 27), (37, 58)], 4
    raw = torch.from_numpy(synth.normal("rectref/raw", (2, 3 * (5 + nc), 6, 6))).double()
    whole = darknet_ref.yolo_decode(raw.float(), anchors, nc, 6 * 32).view(2, 3, 6, 6, 5 + nc)
    for gh, gw in ((1, 4), (4, 1), (2, 3), (3, 2), (5, 6)):
        rows, _ = rect_refs.yolo_decode_rect(raw[:, :, :gh, :gw].contiguous(), anchors, nc, (gh * 32, gw * 32))
        ph.assert_close(rows.view(2, 3, gh, gw, 5 + nc), whole[:, :, :gh, :gw], TOL, f"{gh}x{gw}")


@pytest.mark.parametrize("n,s,mode", [(2, 64, 0), (2, 64, 1), (2, 64, 2), (2, 96, 0), (2, 96, 2)])
def test_network_forward_rect_equals_the_oracle_on_square_frames(n, s, mode):
    from oracle import network_ref
    from millieye_amd.my_models import Network, define_yolo
    conf = 0.2
    net = Network(define_yolo(ph.cfg_path(NAME)), conf).eval()
    synth.fill_network_(net, f"rectref/net/{s}")
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    x = ph.frames(f"rectref/net/{s}/x", n, s)
    maps, rboxes = synth.radar_inputs(f"rectref/net/{s}/radar", n, s // 16)
    maps, rboxes = torch.from_numpy(maps), torch.from_numpy(rboxes)
    ref = network_ref.network_forward(cfgs.KNOWN[NAME](), sd, x, maps, rboxes, mode, conf_thresh=conf)
    got, scaled = rect_refs.network_forward_rect(net, x, maps, rboxes, mode, conf_thresh=conf)
    assert torch.equal(scaled[:, 1:], rboxes[:, 1:] * s) and torch.equal(scaled[:, 0], rboxes[:, 0])
    assert got.shape == ref.shape and got.shape[0] > 0
    assert torch.equal(got[:, 0], ref[:, 0])
    ph.assert_close(got, ref, TOL, f"mode {mode} rows")


@pytest.mark.parametrize("name,n,h,w", [(NAME, n, h, w) for n in (1, 3) for h, w in ((64, 96), (96, 64), (32, 128), (128, 32))]
                         + [("yolov3", 1, 64, 96)])
def test_border_rows_stay_under_the_cap_of_the_cell_test(name, n, h, w):
    """The GPU cell test excludes rows whose sigmoid rounded onto a cell border, at most 1 % of them: the seeded cases stay
    under that cap in float64, and their row order gives the cells it expects."""
    model, x, fm, rows, frac = rect_refs.detector_case(name, n, h, w)
    edge = rect_refs.edge_rows(frac)
    assert float(edge.double().mean()) <= 0.01
    assert tuple(fm.shape) == (n, fm.shape[1], h // 16, w // 16)
    stride, gx, gy = rect_refs.row_cells(model, h, w)
    assert rows.shape[1] == stride.numel() == sum(l.num_anchors * (h // s) * (w // s)
                                                  for l, s in zip(model.yolo_layers, rect_refs._yolo_strides(model.module_defs)))
    assert torch.equal(torch.floor(rows[..., 0] / stride)[~edge], gx.expand(n, -1)[~edge].double())
    assert torch.equal(torch.floor(rows[..., 1] / stride)[~edge], gy.expand(n, -1)[~edge].double())
