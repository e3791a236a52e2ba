"""The float64 references of tests/train_block_refs.py against torch float64 AUTOGRAD of the stock ops, so that the yardstick
of tests/test_gpu_train_blocks.py is itself checked without a GPU.  Tolerance 1e-12 of each tensor's largest magnitude (two
float64 evaluations of the same formula in different orders); integer-valued cases must agree exactly."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import train_block_refs as R


def _rng(seed):
    return np.random.RandomState(seed)


def _close(got, ref, tol=1e-12):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if got.size else 0.0
    assert err <= tol * max(1.0, float(np.abs(ref).max()) if ref.size else 1.0), err


def _nchw(a_rows_c):
    """[rows, c] -> [1, c, rows, 1] (what BatchNorm2d normalises over)."""
    return torch.from_numpy(np.ascontiguousarray(a_rows_c.T)).reshape(1, a_rows_c.shape[1], a_rows_c.shape[0], 1)


def _rows(t):
    return t.detach().reshape(t.shape[1], t.shape[2]).t().numpy()


@pytest.mark.parametrize("ta,tb", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gemm_and_colsum_refs(ta, tb):
    r = _rng(1)
    m, n, k = 5, 7, 9
    a, b, c = r.randn(*((k, m) if ta else (m, k))), r.randn(*((n, k) if tb else (k, n))), r.randn(m, n)
    ta_, tb_ = torch.from_numpy(a), torch.from_numpy(b)
    want = torch.addmm(torch.from_numpy(c), ta_.t() if ta else ta_, tb_.t() if tb else tb_, beta=-0.5, alpha=1.5).numpy()
    _close(R.gemm(ta, tb, 1.5, a, b, -0.5, c), want)
    _close(R.gemm(ta, tb, 1.0, a, b, 0.0, np.full((m, n), np.nan)), ((a.T if ta else a) @ (b.T if tb else b)))
    assert R.gemm(0, 0, 2.0, np.zeros((3, 0)), np.zeros((0, 4)), 3.0, np.ones((3, 4))).tolist() == (3 * np.ones((3, 4))).tolist()
    _close(R.colsum(c), torch.from_numpy(c).sum(0).numpy())
    assert R.colsum(np.zeros((0, 4))).tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("act", [R.LINEAR, R.LEAKY])
@pytest.mark.parametrize("rows,c,shift", [(2, 3, 0.0), (65, 10, 3.0), (300, 4, 100.0)])
def test_bn_train_refs(rows, c, shift, act):
    r = _rng(rows)
    x, dy = r.randn(rows, c) + shift, r.randn(rows, c)
    gamma, beta = r.uniform(-1.5, 1.5, c), r.uniform(-0.5, 0.5, c)
    rm, rv = r.randn(c), r.uniform(0.5, 1.5, c)
    eps, mom = 1e-5, 0.03
    xt = _nchw(x).requires_grad_(True)
    gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
    rmt, rvt = torch.from_numpy(rm.copy()), torch.from_numpy(rv.copy())
    z = F.batch_norm(xt, rmt, rvt, gt, bt, True, mom, eps)
    y = F.leaky_relu(z, R.SLOPE) if act == R.LEAKY else z
    y.backward(_nchw(dy))
    f = R.bn_train_fwd(x, gamma, beta, eps, mom, rm, rv, act)
    _close(f["y"], _rows(y), 1e-11)
    _close(f["running_mean"], rmt.numpy())
    _close(f["running_var"], rvt.numpy(), 1e-11)
    _close(f["mean"], x.mean(0))
    _close(f["var"], x.var(0), 1e-11)
    b = R.bn_train_bwd(x, dy, gamma, beta, eps, act)
    _close(b["dx"], _rows(xt.grad), 1e-10)
    _close(b["dgamma"], gt.grad.numpy(), 1e-11)
    _close(b["dbeta"], bt.grad.numpy(), 1e-11)
    assert R.bn_train_fwd(x, gamma, beta, eps, mom, None, None, act)["running_mean"] is None


@pytest.mark.parametrize("act", [R.LINEAR, R.LEAKY])
@pytest.mark.parametrize("bn", [True, False])
def test_affine_act_bwd_ref(act, bn):
    r = _rng(7)
    rows, c = 40, 6
    cv, dy = r.randn(rows, c), r.randn(rows, c)
    ct = _nchw(cv).requires_grad_(True)
    if bn:
        gamma, beta = r.uniform(-1.5, 1.5, c), r.uniform(-0.5, 0.5, c)
        rm, rv = r.randn(c), r.uniform(0.5, 1.5, c)
        gt, bt = torch.from_numpy(gamma).requires_grad_(True), torch.from_numpy(beta).requires_grad_(True)
        z = F.batch_norm(ct, torch.from_numpy(rm), torch.from_numpy(rv), gt, bt, False, 0.1, 1e-5)
        scale = gamma / np.sqrt(rv + 1e-5)
        shift = beta - rm * scale
    else:
        bias = r.randn(c)
        bt = torch.from_numpy(bias).requires_grad_(True)
        z = ct + bt.view(1, c, 1, 1)
        scale, shift, gamma, beta = None, bias, None, None
    y = F.leaky_relu(z, R.SLOPE) if act == R.LEAKY else z
    y.backward(_nchw(dy))
    got = R.affine_act_bwd(cv, dy, scale, shift, gamma, beta, act)
    _close(got["dc"], _rows(ct.grad))
    _close(got["dshift"], bt.grad.numpy())
    if bn:
        _close(got["dgamma"], gt.grad.numpy(), 1e-11)
    else:
        assert got["dgamma"] is None


def test_leaky_slope_at_zero_and_sigmoid_ref():
    x = torch.tensor([[-2.0, 0.0, 3.0]], dtype=torch.float64, requires_grad=True)
    y = F.leaky_relu(x, R.SLOPE)
    y.backward(torch.ones_like(y))
    assert R.act_bwd(y.detach().numpy(), np.ones((1, 3)), R.LEAKY).tolist() == x.grad.numpy().tolist() == [[R.SLOPE, R.SLOPE, 1.0]]
    assert R.act_bwd(y.detach().numpy(), np.ones((1, 3)), R.LINEAR).tolist() == [[1.0, 1.0, 1.0]]
    xs = torch.from_numpy(_rng(3).randn(9, 5) * 3).requires_grad_(True)
    ys = torch.sigmoid(xs)
    dy = _rng(4).randn(9, 5)
    ys.backward(torch.from_numpy(dy))
    _close(R.act_bwd(ys.detach().numpy(), dy, R.SIGMOID), xs.grad.numpy())
    assert R.SLOPE == float(torch.tensor(0.1, dtype=torch.float32))


@pytest.mark.parametrize("n,h,w,c", [(1, 1, 1, 1), (2, 3, 5, 4)])
def test_upsample2_bwd_ref(n, h, w, c):
    dy = _rng(h).randint(-4, 5, (n, 2 * h, 2 * w, c)).astype(np.float64)
    x = torch.zeros(n, c, h, w, dtype=torch.float64, requires_grad=True)
    F.interpolate(x, scale_factor=2, mode="nearest").backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.array_equal(R.upsample2_bwd(dy), x.grad.permute(0, 2, 3, 1).numpy())


@pytest.mark.parametrize("size,stride,pad,zero_ext", [(2, 2, 0, 0), (2, 1, 0, 1), (3, 1, 1, 0), (5, 1, 2, 0)])
@pytest.mark.parametrize("h,w", [(6, 8), (5, 7), (2, 3)])
@pytest.mark.parametrize("data", ["ties", "negative", "real"])
def test_maxpool_bwd_ref(size, stride, pad, zero_ext, h, w, data):
    """Includes the two rules the kernel's comment claims: a tie goes to the first maximum in row-major order, and a padded zero
    that wins (all-negative window under the zero extension) receives nothing - both are what torch's CPU backward does."""
    r = _rng(10 * h + size)
    n, c = 2, 3
    if data == "ties":
        x = r.randint(-2, 3, (n, h, w, c)).astype(np.float64)
        x[0, : h // 2] = 1.0   # a constant patch
    elif data == "negative":
        x = -r.randint(1, 4, (n, h, w, c)).astype(np.float64)
    else:
        x = r.randn(n, h, w, c)
    ho, wo = R.maxpool_out_size(h, size, stride, pad, zero_ext), R.maxpool_out_size(w, size, stride, pad, zero_ext)
    dy = r.randint(-4, 5, (n, ho, wo, c)).astype(np.float64)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    xin = F.pad(xt, (0, 1, 0, 1), value=0.0) if zero_ext else xt
    y = F.max_pool2d(xin, size, stride, pad)
    assert tuple(y.shape[2:]) == (ho, wo)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    got = R.maxpool_bwd(x, dy, size, stride, pad, zero_ext)
    assert np.array_equal(got, xt.grad.permute(0, 2, 3, 1).numpy())
    if data == "negative" and zero_ext:
        # every window that touches the zero border is won by a zero, which receives nothing: its gradient is dropped
        assert got.sum() == dy[:, :h - 1, :w - 1, :].sum()


@pytest.mark.parametrize("n,h,w,cin,cout,k,s", [(2, 5, 6, 3, 4, 3, 1), (1, 7, 7, 2, 5, 3, 2), (2, 4, 4, 6, 3, 1, 1), (1, 8, 8, 2, 2, 5, 1)])
def test_conv_wgrad_ref(n, h, w, cin, cout, k, s):
    r = _rng(k)
    pad = (k - 1) // 2
    x = r.randint(-4, 5, (n, h, w, cin)).astype(np.float64)
    wt = torch.zeros(cout, cin, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), wt, None, s, pad)
    dy = r.randint(-4, 5, tuple(y.permute(0, 2, 3, 1).shape)).astype(np.float64)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.array_equal(R.conv_wgrad(x, dy, k, s, pad), wt.grad.numpy())


@pytest.mark.parametrize("m", [0, 5])
def test_yolo_loss_grad_ref(m):
    """Autograd through the restated terms against autograd through ``oracle/darknet_ref.yolo_loss`` (the reference's own
    statements, pinned by tests/golden/yololoss_*.npz), with the dense tensors of ``yolo_loss_terms``."""
    from oracle import darknet_ref
    r = _rng(11)
    n, g, nc = 2, 6, 4
    anchors = [(10, 13), (33, 23), (62, 45)]
    raw = r.normal(0, 1.5, (n, g, g, 3 * (5 + nc))).astype(np.float32)
    tg = np.zeros((m, 6), np.float32)
    if m:
        tg[:, 0], tg[:, 1] = r.randint(0, n, m), r.randint(0, nc, m)
        tg[:, 2:4], tg[:, 4:6] = r.uniform(0.02, 0.98, (m, 2)), r.uniform(0.03, 0.5, (m, 2))
    _loss, _metrics, dense = darknet_ref.yolo_loss_terms(torch.from_numpy(raw), anchors, nc, 32 * g, torch.from_numpy(tg))
    dense = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in dense.items()}
    got = R.yolo_loss_grad(raw, dense, 3, nc, 1.0, 100.0, grad_scale=0.25)
    assert got.dtype == np.float64 and np.isfinite(got).all()
    neither = ~(dense["obj"] | dense["noobj"])
    cells = got.reshape(n, g, g, 3, nc + 5).transpose(0, 3, 1, 2, 4)
    assert np.all(cells[neither] == 0)
    got32 = R.yolo_loss_grad(raw, dense, 3, nc, 1.0, 100.0, grad_scale=0.25, dtype=torch.float32)
    assert got32.dtype == np.float32
    _close(got32, got, 1e-5)
    if m:   # (yolo_loss builds float32 tensors: it runs in single precision only)
        rt = torch.from_numpy(raw).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        loss = darknet_ref.yolo_loss(rt, anchors, nc, 32 * g, torch.from_numpy(tg))
        (loss * 0.25).backward()
        _close(got, rt.grad.permute(0, 2, 3, 1).numpy(), 1e-5)
