"""Plain float64 references of the training building blocks (csrc/train.hip, csrc/train_h16.hip): one small function per
operation, numpy / torch float64 only, no project kernel.  Layouts are the kernels': matrices are [rows, channels], maps are
NHWC.  ``tests/test_train_block_refs_cpu.py`` pins every function to torch float64 autograd of the stock op, and
``tests/test_gpu_train_blocks.py`` compares the kernels with them.

The LeakyReLU slope is the float32 value of 0.1 (what ``F.leaky_relu(x_f32, 0.1)`` and the kernels' ``0.1f`` multiply with),
and a pre-activation of exactly 0 takes the slope (torch: ``x > 0 ? 1 : slope``)."""
import numpy as np
import torch

LINEAR, LEAKY, SIGMOID = 0, 1, 2
SLOPE = float(np.float32(0.1))


def _f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def gemm(trans_a, trans_b, alpha, a, b, beta=0.0, c=None):
    """alpha * op(A) op(B) + beta * C; C is not read when beta == 0."""
    a, b = _f64(a), _f64(b)
    p = (a.T if trans_a else a) @ (b.T if trans_b else b)
    out = alpha * p
    if beta != 0.0:
        out = out + beta * _f64(c)
    return out


def gemm_abs(trans_a, trans_b, a, b):
    """sum_k |a| |b| per element: the scale of the rounding-error bound of a length-k dot product."""
    a, b = np.abs(_f64(a)), np.abs(_f64(b))
    return (a.T if trans_a else a) @ (b.T if trans_b else b)


def colsum(x):
    return _f64(x).sum(0)


def act_grad(pre_or_out, act):
    """act'(.) as a factor; for LeakyReLU the sign of the pre-activation and of the output agree, so either may be given."""
    v = _f64(pre_or_out)
    if act == LEAKY:
        return np.where(v > 0, 1.0, SLOPE)
    if act == LINEAR:
        return np.ones_like(v)
    raise ValueError(act)


def act_bwd(y, dy, act):
    """dx = dy * act'(.) from the activation OUTPUT y (sigmoid: y (1 - y))."""
    y, dy = _f64(y), _f64(dy)
    if act == SIGMOID:
        return dy * y * (1.0 - y)
    return dy * act_grad(y, act)


def bn_train_fwd(x, gamma, beta, eps, momentum, running_mean, running_var, act):
    """nn.BatchNorm2d in training mode over the rows of x [rows, channels], two-pass variance.  Returns a dict with y, mean,
    var (biased), rstd and the updated running statistics (None without them)."""
    x, gamma, beta = _f64(x), _f64(gamma), _f64(beta)
    rows = x.shape[0]
    mean = x.sum(0) / rows
    var = ((x - mean) ** 2).sum(0) / rows
    rstd = 1.0 / np.sqrt(var + eps)
    z = (x - mean) * rstd * gamma + beta
    y = np.where(z > 0, z, SLOPE * z) if act == LEAKY else z
    out = dict(y=y, mean=mean, var=var, rstd=rstd, z=z, running_mean=None, running_var=None)
    if running_mean is not None:
        unbiased = var * rows / (rows - 1) if rows > 1 else var
        out["running_mean"] = (1.0 - momentum) * _f64(running_mean) + momentum * mean
        out["running_var"] = (1.0 - momentum) * _f64(running_var) + momentum * unbiased
    return out


def bn_train_bwd(x, dy, gamma, beta, eps, act):
    """Gradient of ``act(batch_norm(x))`` (batch statistics) w.r.t. x, gamma, beta; dy is the gradient of the activated output."""
    f = bn_train_fwd(x, gamma, beta, eps, 0.0, None, None, act)
    x, gamma = _f64(x), _f64(gamma)
    rows = x.shape[0]
    xhat = (x - f["mean"]) * f["rstd"]
    g = _f64(dy) * act_grad(f["z"], act)
    dbeta = g.sum(0)
    dgamma = (g * xhat).sum(0)
    dx = gamma * f["rstd"] * (g - dbeta / rows - xhat * dgamma / rows)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def affine_act_bwd(c, dy, scale, shift, gamma, beta, act):
    """Backward of the eval-mode conv block ``y = act(scale * c + shift)`` (scale = gamma * rstd, shift = beta - mean * scale;
    scale None = 1, shift None = 0): dc, dshift = sum g, and - with gamma - dgamma = sum g * xhat, xhat = (z - beta) / gamma from
    the PRE-ACTIVATION z = scale * c + shift (what autograd differentiates), never from a stored, rounded output."""
    c, dy = _f64(c), _f64(dy)
    s = _f64(scale) if scale is not None else np.ones(c.shape[1])
    z = c * s + (_f64(shift) if shift is not None else 0.0)
    g = dy * act_grad(z, act)
    out = dict(dc=g * s, dshift=g.sum(0), dgamma=None, z=z, g=g)
    if gamma is not None:
        out["dgamma"] = (g * ((z - _f64(beta)) / _f64(gamma))).sum(0)
    return out


def upsample2_bwd(dy):
    """Gradient of nearest x2 upsampling: 2x2 block sums of dy [n, 2h, 2w, c]."""
    dy = _f64(dy)
    n, h2, w2, c = dy.shape
    return dy.reshape(n, h2 // 2, 2, w2 // 2, 2, c).sum((2, 4))


def maxpool_out_size(h, size, stride, pad, zero_ext):
    return (h + (1 if zero_ext else 0) + 2 * pad - size) // stride + 1


def maxpool_bwd(x, dy, size, stride, pad, zero_ext):
    """Gradient of max pooling over x [n, h, w, c]: every output's gradient goes to the FIRST maximum of its window in row-major
    order.  ``pad`` cells never win (-inf); ``zero_ext`` is darknet's ZeroPad2d((0, 1, 0, 1)) in front of the pool: one more row
    and column of zeros at the bottom / right, which can win and then receive nothing."""
    x, dy = _f64(x), _f64(dy)
    n, h, w, c = x.shape
    ext = 1 if zero_ext else 0
    ho, wo = maxpool_out_size(h, size, stride, pad, zero_ext), maxpool_out_size(w, size, stride, pad, zero_ext)
    assert dy.shape == (n, ho, wo, c), (dy.shape, (n, ho, wo, c))
    big = np.full((n, h + ext + 2 * pad, w + ext + 2 * pad, c), -np.inf)
    big[:, pad:pad + h + ext, pad:pad + w + ext, :] = 0.0
    big[:, pad:pad + h, pad:pad + w, :] = x
    dbig = np.zeros_like(big)
    ni, ci = np.meshgrid(np.arange(n), np.arange(c), indexing="ij")
    for oy in range(ho):
        for ox in range(wo):
            win = big[:, oy * stride:oy * stride + size, ox * stride:ox * stride + size, :]
            flat = win.transpose(0, 3, 1, 2).reshape(n, c, size * size)
            arg = flat.argmax(-1)   # numpy: the first occurrence of the maximum
            np.add.at(dbig, (ni, oy * stride + arg // size, ox * stride + arg % size, ci), dy[:, oy, ox, :])
    return dbig[:, pad:pad + h, pad:pad + w, :]


def conv_wgrad(x, dy, ksize, stride, pad):
    """dW [cout, cin, k, k] of y = conv2d(x, W) from x [n, h, w, cin] and dy [n, ho, wo, cout] (zero padding)."""
    x, dy = _f64(x), _f64(dy)
    n, h, w, cin = x.shape
    _, ho, wo, cout = dy.shape
    xp = np.zeros((n, h + 2 * pad, w + 2 * pad, cin))
    xp[:, pad:pad + h, pad:pad + w, :] = x
    dw = np.zeros((cout, cin, ksize, ksize))
    d2 = dy.reshape(-1, cout)
    for ky in range(ksize):
        for kx in range(ksize):
            xs = xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride, :]
            dw[:, :, ky, kx] = d2.T @ xs.reshape(-1, cin)
    return dw


def yolo_loss_grad(raw_nhwc, dense, num_anchors, num_classes, obj_scale, noobj_scale, grad_scale=1.0, dtype=torch.float64):
    """d(grad_scale * loss) / d(raw) of one YOLO layer by autograd through the formulae of ``oracle/darknet_ref.yolo_loss_terms``
    (mse of x, y, w, h over the object cells, bce of the confidence over object / no-object cells, bce of the classes), from
    the raw map [N, G, G, A*(5+C)] and the dense build_targets tensors (obj / noobj [N,A,G,G], tx, ty, tw, th, tconf, tcls).
    ``dtype=torch.float32`` is the same restatement in single precision (the yardstick of the kernels' error bar).  A term
    over an empty selection (the reference's NaN mean) contributes no gradient and is left out."""
    import torch.nn.functional as F
    raw = torch.as_tensor(np.asarray(raw_nhwc)).to(dtype).clone().requires_grad_(True)
    n, g = raw.shape[0], raw.shape[1]
    pred = raw.reshape(n, g, g, num_anchors, num_classes + 5).permute(0, 3, 1, 2, 4)
    x, y = torch.sigmoid(pred[..., 0]), torch.sigmoid(pred[..., 1])
    w, h = pred[..., 2], pred[..., 3]
    conf, cls = torch.sigmoid(pred[..., 4]), torch.sigmoid(pred[..., 5:])
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in dense.items() if k not in ("n_obj", "n_noobj")}
    obj, noobj = t["obj"].bool(), t["noobj"].bool()
    tx, ty, tw, th, tconf, tcls = (t[k].to(dtype) for k in ("tx", "ty", "tw", "th", "tconf", "tcls"))
    loss = raw.sum() * 0
    if bool(obj.any()):
        loss = loss + F.mse_loss(x[obj], tx[obj]) + F.mse_loss(y[obj], ty[obj]) + F.mse_loss(w[obj], tw[obj]) + \
            F.mse_loss(h[obj], th[obj]) + obj_scale * F.binary_cross_entropy(conf[obj], tconf[obj]) + \
            F.binary_cross_entropy(cls[obj], tcls[obj])
    if bool(noobj.any()):
        loss = loss + noobj_scale * F.binary_cross_entropy(conf[noobj], tconf[noobj])
    (loss * grad_scale).backward()
    return raw.grad.numpy()
