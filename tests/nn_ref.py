"""The latent-space integrator (arch='nn') restated in NumPy, twice: ``Ops64`` in fp64 and ``Ops32``, an op-for-op fp32 twin with the
summation orders of include/deepfluids_hip_nn.h and the same hash mask.  TensorFlow is not available, so no golden was captured from
the reference's ``NN``: parity is with this restatement of model.py:218-224, trainer.py:586-747 and data_nn.py:62-126.

What the twin reproduces bit for bit: the mask, the column sums (so mean, rstd and the moving averages given the same input), the backward
block, the window advance, the MSE.  Its linear layers follow df_linear_fwd / df_linear_bwd of the main library op for op as well (the
general path, taken below K = 1024 or above N = 32: a chain of fused multiply-adds over k, or over the batch for the weight gradient; the
bias gradient added row by row; the input gradient accumulated in fp64), with a fused multiply-add formed as the fp64 product -- exact --
plus the accumulator, rounded to fp32: equal to the device's up to a double rounding on exact ties.  ELU is the header's own fp32
series, repeated here step by step (fp64: the true exp(y) - 1).  Everything downstream of ELU is compared to fp64 with ``tolerance``
below."""
import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32
M1, M2, M3 = U32(0x8DA6B343), U32(0xD8163841), U32(0xCB1AB31F)
EPS, DECAY = 1e-5, 0.9
NAMES = ["fully_connected/weights", "fully_connected/biases", "BatchNorm/beta", "BatchNorm/gamma", "BatchNorm/moving_mean",
         "BatchNorm/moving_variance", "fully_connected_1/weights", "fully_connected_1/biases", "BatchNorm_1/beta", "BatchNorm_1/gamma",
         "BatchNorm_1/moving_mean", "BatchNorm_1/moving_variance", "fully_connected_2/weights", "fully_connected_2/biases"]
FC = ["fully_connected", "fully_connected_1", "fully_connected_2"]
BN = ["BatchNorm", "BatchNorm_1"]
TRAINABLE = [n for n in NAMES if "moving" not in n]


def mix(h):
    h = np.array(h, dtype=U32, ndmin=1)
    h ^= h >> U32(16); h *= U32(0x7FEB352D); h ^= h >> U32(15); h *= U32(0x846CA68B); h ^= h >> U32(16)
    return h


def mask_key(seed, step, window, layer):
    a = lambda v: np.array([int(v) & 0xFFFFFFFF], dtype=U32)
    return mix(a(seed) ^ (a(step) * M1) ^ (a(window) * M2) ^ (a(layer) * M3))


def mask(key, B, N, keep_prob, row0=0, col0=0):
    """kept [B,N] (bool) of rows row0.. and columns col0..: a function of the element's own row and column only"""
    r = (np.arange(row0, row0 + B, dtype=np.int64).astype(U32) * M1)[:, None]
    c = (np.arange(col0, col0 + N, dtype=np.int64).astype(U32) * M2)[None, :]
    h = mix(key ^ r ^ c)
    return (h >> U32(8)).astype(F32) * F32(2.0 ** -24) < F32(keep_prob)


def tolerance(ref64, twin32):
    """4 x the twin's own deviation from fp64 (largest absolute difference over the tensor), and never below 4 x one fp32 rounding of the
    tensor's largest magnitude: the result is stored as fp32, so a deviation of zero in the twin (a tiny tensor, an exact value) is
    no license to demand the fp64 value to more digits than the format holds."""
    ref64 = np.asarray(ref64, F64)
    dev = float(np.abs(np.asarray(twin32, F64) - ref64).max()) if ref64.size else 0.0
    return 4.0 * max(dev, float(np.finfo(F32).eps) * float(np.abs(ref64).max() if ref64.size else 0.0))


class Ops64(object):
    dt = F64

    def arr(self, a):
        return np.array(a, dtype=self.dt)

    def colsum(self, a):
        return a.sum(axis=0)

    def linear(self, x, w, b):
        return x @ w + b

    def linear_bwd(self, x, w, gy):
        return gy @ w.T, x.T @ gy, gy.sum(axis=0)

    def stats(self, x):
        B = x.shape[0]
        mean = self.colsum(x) / B
        d = x - mean
        var = self.colsum(d * d) / B
        return mean, var, 1.0 / np.sqrt(var + F64(F32(EPS)))

    def elu(self, y):
        return np.where(y > 0, y, np.expm1(np.minimum(y, 0)))

    def bn_fwd(self, x, gamma, beta, mm, mv, kept, keep_prob, decay=DECAY):
        """-> out, act, mean, rstd, new moving mean, new moving variance"""
        dt = self.dt
        B = x.shape[0]
        mean, var, rstd = self.stats(x)
        act = self.elu(((x - mean) * rstd) * gamma + beta)
        inv = dt(1) / dt(F32(keep_prob))
        out = np.where(kept, act * inv, dt(0))
        decay = dt(F32(decay)); omd = dt(1) - decay
        bessel = dt(B) / dt(max(B - 1, 1))
        return out, act, mean, rstd, mm * decay + mean * omd, mv * decay + (var * bessel) * omd

    def bn_bwd(self, x, act, gout, gamma, mean, rstd, kept, keep_prob):
        """-> gx, ggamma, gbeta"""
        dt = self.dt
        B = x.shape[0]
        inv = dt(1) / dt(F32(keep_prob))
        gd = np.where(kept, gout * inv, dt(0))
        dy = np.where(act < 0, gd * (act + dt(1)), gd)
        xh = (x - mean) * rstd
        gb, gg = self.cast(self.colsum(dy)), self.cast(self.colsum(dy * xh))
        ib = dt(1) / dt(B)
        return (gamma * rstd) * ((dy - gb * ib) - xh * (gg * ib)), gg, gb

    def cast(self, a):
        return a

    def bn_infer(self, x, gamma, beta, mm, mv):
        rstd = self.cast(1.0 / np.sqrt(mv.astype(F64) + F64(F32(EPS))))
        return self.elu(((x - mm) * rstd) * gamma + beta)

    def advance(self, x, y, xw, i, ratio, z):
        return np.concatenate([x[:, :z] + y * self.dt(ratio), xw[:, i + 1, z:]], axis=1)

    def mse(self, a, b):
        d = a - b
        return (d * d).mean()

    def mse_bwd(self, a, b, gout=1.0):
        return (self.dt(gout) * (self.dt(2) / self.dt(a.size))) * (a - b)

    def matvec(self, v, w, b):
        return v @ w + b


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in fp64"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


class Ops32(Ops64):
    dt = F32

    def cast(self, a):
        return np.asarray(a).astype(F32)

    @staticmethod
    def _general_path(K, N):
        assert not (N <= 32 and K >= 1024), "the twin follows df_linear_*'s general path only (K < 1024 or N > 32)"

    def linear(self, x, w, b):
        """linear_fwd_kernel: acc = fmaf(x[b,k], w[k,n], acc) for k ascending from 0, then + bias"""
        self._general_path(*w.shape)
        acc = np.zeros((x.shape[0], w.shape[1]), F32)
        for k in range(w.shape[0]):
            acc = _fma(x[:, k:k + 1], w[k][None, :], acc)
        return acc + b

    def linear_bwd(self, x, w, gy):
        """linear_bwd_w_kernel: gw[k,n] = fmaf(x[b,k], gy[b,n], acc) and gb[n] += gy[b,n] for b ascending; linear_bwd_x_kernel: the
        products of gy[b,:] and w[k,:] added in fp64, rounded once"""
        self._general_path(*w.shape)
        gw, gb = np.zeros(w.shape, F32), np.zeros(w.shape[1], F32)
        for b in range(x.shape[0]):
            gw = _fma(x[b][:, None], gy[b][None, :], gw)
            gb = gb + gy[b]
        return (gy.astype(F64) @ w.astype(F64).T).astype(F32), gw, gb

    def elu(self, y):
        """elu of the header, step by step"""
        y = np.asarray(y, F32)
        with np.errstate(invalid="ignore", over="ignore"):
            n = np.rint(y * F32(1.44269502))
            r = (y - n * F32(0.693359375)) - n * F32(-2.12194440e-4)
            q = np.full_like(r, F32(2.48015873e-5))
            for c in (1.98412698e-4, 1.38888889e-3, 8.33333333e-3, 4.16666667e-2, 1.66666667e-1, 0.5):
                q = q * r + F32(c)
            p = r + (r * r) * q
            s = np.ldexp(F32(1), np.clip(n, -200, 200).astype(np.int32)).astype(F32)
            e = s * p + (s - F32(1))
        return np.where(y > 0, y, np.where(y < F32(-17.5), F32(-1), e)).astype(F32)

    def colsum(self, a):
        """S(.) of the header: 32 row threads per column, fp32 ascending each, then fp64 ascending -> fp64 [N]"""
        tot = np.zeros(a.shape[1], F64)
        for q in range(32):
            acc = np.zeros(a.shape[1], F32)
            for row in a[q::32]:
                acc = acc + row
            tot = tot + acc.astype(F64)
        return tot

    def stats(self, x):
        B = x.shape[0]
        mean = (self.colsum(x) / F64(B)).astype(F32)
        d = x - mean
        var = (self.colsum(d * d) / F64(B)).astype(F32)
        return mean, var, (1.0 / np.sqrt(var.astype(F64) + F64(F32(EPS)))).astype(F32)

    @staticmethod
    def _tree(v):
        """[..., 256] fp64 -> [...]: the tree inside each wave, then the four waves ascending"""
        v = v.reshape(v.shape[:-1] + (4, 64)).copy()
        off = 32
        while off:
            v[..., :off] = v[..., :off] + v[..., off:2 * off]
            off >>= 1
        w = v[..., 0]
        return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]

    def mse(self, a, b):
        d = (a - b).reshape(-1)
        n = d.size
        nblk = -(-n // 1024)
        sq = np.zeros(nblk * 1024, F32)
        sq[:n] = d * d
        sq = sq.reshape(nblk, 4, 256)
        acc = np.zeros((nblk, 256), F32)
        for i in range(4):
            acc = acc + sq[:, i]
        part = self._tree(acc.astype(F64))                      # [nblk]
        pad = np.zeros(-(-nblk // 256) * 256, F64)
        pad[:nblk] = part
        t = np.zeros(256, F64)
        for chunk in pad.reshape(-1, 256):
            t = t + chunk
        return F32(self._tree(t) / F64(n))

    def mse_bwd(self, a, b, gout=1.0):
        return (F32(gout) * (F32(2) / F32(a.size))) * (a - b)

    def matvec(self, v, w, b):
        """the rollout's matrix-vector product: chunks of 1024 columns, k in 1024 // nb interleaved parts"""
        K, N = w.shape
        out = np.zeros(N, F32)
        for n0 in range(0, N, 1024):
            nb = min(N - n0, 1024)
            sk = 1024 // nb
            tot = np.zeros(nb, F64)
            for q in range(sk):
                acc = np.zeros(nb, F32)
                for k in range(q, K, sk):
                    acc = acc + v[k] * w[k, n0:n0 + nb]
                tot = tot + acc.astype(F64)
            out[n0:n0 + nb] = tot.astype(F32) + b[n0:n0 + nb]
        return out


def matvec_chunks(K, N):
    """the branches ``Ops32.matvec`` (and ``matvec`` of rollout_kernel) takes for a [K,N] layer: per chunk of 1024 columns
    ``(n0, nb, sk, idle)`` -- its first column, its columns, the interleaved parts of k, and the threads of the workgroup beyond
    sk * nb, which hold no partial sum"""
    out = []
    for n0 in range(0, N, 1024):
        nb = min(N - n0, 1024)
        sk = 1024 // nb
        out.append((n0, nb, sk, 1024 - sk * nb))
    return out


def init_params(rng, k0, filters, z_num, scale=1.0, n2=None):
    """fp64 parameters under the slim names (Xavier-uniform weights times ``scale``; biases, beta, gamma and the moving statistics drawn
    too, so that no term of a test is hidden behind a zero or a one).  ``n2``: the second hidden width where it is not ``filters``
    (the first is 2 * filters, or ``filters`` itself when ``n2`` is given: the edge tests' N1 / N2 are not tied to each other)"""
    n1, n2 = (2 * filters, filters) if n2 is None else (filters, n2)
    dims = [(k0, n1), (n1, n2), (n2, z_num)]
    p = {}
    for fc, (i, o) in zip(FC, dims):
        lim = np.sqrt(6.0 / (i + o)) * scale
        p[fc + "/weights"] = rng.uniform(-lim, lim, (i, o))
        p[fc + "/biases"] = rng.uniform(-0.1, 0.1, o)
    for bn, (_, o) in zip(BN, dims):
        p[bn + "/beta"] = rng.uniform(-0.2, 0.2, o)
        p[bn + "/gamma"] = rng.uniform(0.8, 1.2, o)
        p[bn + "/moving_mean"] = rng.uniform(-0.2, 0.2, o)
        p[bn + "/moving_variance"] = rng.uniform(0.5, 1.5, o)
    return {k: p[k].astype(F32).astype(F64) for k in NAMES}      # values fp32 holds exactly: both precisions start from the same numbers


def cast_params(ops, p):
    return {k: ops.arr(v) for k, v in p.items()}


def window_step(ops, p, xw, yw, ratio, keep_prob, seed, step, train=True, want_grad=True):
    """The windowed graph of build_model_nn on parameters ``p`` (of ops.dt): -> dict(loss, yw_, grads (by name, trainable only), moving
    (the parameters' moving statistics after the w_num training-mode applications; unchanged in evaluation mode))"""
    dt = ops.dt
    xw, yw = ops.arr(xw), ops.arr(yw)
    B, W, K0 = xw.shape
    z = yw.shape[2]
    p = dict(p)
    x_ = xw[:, 0, :]
    caches, ys = [], []
    for i in range(W):
        c = {"x": [x_], "bn": []}
        h = x_
        for layer, (fc, bn) in enumerate(zip(FC[:2], BN)):
            a = ops.linear(h, p[fc + "/weights"], p[fc + "/biases"])
            if train:
                kept = mask(mask_key(seed, step, i, layer), a.shape[0], a.shape[1], keep_prob)
                h, act, mean, rstd, p[bn + "/moving_mean"], p[bn + "/moving_variance"] = ops.bn_fwd(
                    a, p[bn + "/gamma"], p[bn + "/beta"], p[bn + "/moving_mean"], p[bn + "/moving_variance"], kept, keep_prob)
                c["bn"].append((a, act, mean, rstd, kept))
            else:
                h = ops.bn_infer(a, p[bn + "/gamma"], p[bn + "/beta"], p[bn + "/moving_mean"], p[bn + "/moving_variance"])
            c["x"].append(h)
        y = ops.linear(h, p[FC[2] + "/weights"], p[FC[2] + "/biases"])
        ys.append(y)
        caches.append(c)
        if i < W - 1:
            x_ = ops.advance(x_, y, xw, i, ratio, z)
    yw_ = np.stack(ys, axis=1)
    out = {"loss": ops.mse(yw_, yw), "yw_": yw_, "moving": {k: p[k] for k in NAMES if "moving" in k}}
    if not (train and want_grad):
        return out
    g = {k: np.zeros_like(p[k]) for k in TRAINABLE}
    gyw = ops.mse_bwd(yw_, yw)
    gxn = None
    for i in reversed(range(W)):          # the order autograd accumulates in: the last application first
        c = caches[i]
        gy = gyw[:, i, :]
        if gxn is not None:
            gy = gy + gxn[:, :z] * dt(ratio)
        gh, gw, gb = ops.linear_bwd(c["x"][2], p[FC[2] + "/weights"], gy)
        g[FC[2] + "/weights"] = g[FC[2] + "/weights"] + gw; g[FC[2] + "/biases"] = g[FC[2] + "/biases"] + gb
        for layer in (1, 0):
            fc, bn = FC[layer], BN[layer]
            a, act, mean, rstd, kept = c["bn"][layer]
            ga, gg, gbeta = ops.bn_bwd(a, act, gh, p[bn + "/gamma"], mean, rstd, kept, keep_prob)
            g[bn + "/gamma"] = g[bn + "/gamma"] + gg; g[bn + "/beta"] = g[bn + "/beta"] + gbeta
            gh, gw, gb = ops.linear_bwd(c["x"][layer], p[fc + "/weights"], ga)
            g[fc + "/weights"] = g[fc + "/weights"] + gw; g[fc + "/biases"] = g[fc + "/biases"] + gb
        if i > 0:
            carry = np.zeros_like(gh)
            if gxn is not None:
                carry[:, :z] = gxn[:, :z]
            gxn = gh + carry
    out["grads"] = g
    return out


def adam_state(p):
    return {"m": {k: np.zeros_like(p[k]) for k in TRAINABLE}, "v": {k: np.zeros_like(p[k]) for k in TRAINABLE}, "t": 0}


def adam_step(ops, p, g, st, lr, beta1=0.5, beta2=0.999, eps=1e-8):
    """TF1 Adam ("epsilon-hat"), as df_adam_tf1_step: lr_t on the host in fp64, rounded to the op's precision"""
    dt = ops.dt
    st["t"] += 1
    lr_t = dt(lr * np.sqrt(1.0 - beta2 ** st["t"]) / (1.0 - beta1 ** st["t"]))
    b1, b2, e = dt(F32(beta1)), dt(F32(beta2)), dt(F32(eps))
    for k in TRAINABLE:
        st["m"][k] = b1 * st["m"][k] + (dt(1) - b1) * g[k]
        st["v"][k] = b2 * st["v"][k] + ((dt(1) - b2) * g[k]) * g[k]          # adam_kernel's association
        p[k] = p[k] - lr_t * st["m"][k] / (np.sqrt(st["v"][k]) + e)
    return p


def train_steps(ops, p, batches, ratio, keep_prob, seed, lr_of_step, step0=0):
    """``len(batches)`` optimizer steps from fp64 parameters ``p``: -> (parameters after the last step, [window_step result per step])"""
    p = cast_params(ops, p)
    st = adam_state(p)
    outs = []
    for s, (xw, yw) in enumerate(batches):
        r = window_step(ops, p, xw, yw, ratio, keep_prob, seed, step0 + s)
        p.update(r["moving"])
        p = adam_step(ops, p, r["grads"], st, lr_of_step(step0 + s))
        outs.append(r)
    return p, outs


def forward_eval(ops, p, x):
    """NN(x, train=False)"""
    h = ops.arr(x)
    for fc, bn in zip(FC[:2], BN):
        h = ops.bn_infer(ops.linear(h, p[fc + "/weights"], p[fc + "/biases"]), p[bn + "/gamma"], p[bn + "/beta"], p[bn + "/moving_mean"],
                         p[bn + "/moving_variance"])
    return ops.linear(h, p[FC[2] + "/weights"], p[FC[2] + "/biases"])


def rollout(ops, p, x_test, y_test, S, F, z, code_std, out_std):
    """test_nn (trainer.py:698-747): -> z_out [S,F,z]; the matrix-vector products in the order of the rollout kernel"""
    dt = ops.dt
    x_test, y_test = ops.arr(x_test), ops.arr(y_test)
    cs, os_ = dt(F32(code_std)), dt(F32(out_std))
    pn = x_test.shape[1] - z
    rs = [ops.cast(1.0 / np.sqrt(p[bn + "/moving_variance"].astype(F64) + F64(F32(EPS)))) for bn in BN]
    z_out = np.zeros((S, F, z), dt)
    for s in range(S):
        xin = x_test[s * (F - 1)].copy()
        z_out[s, 0] = xin[:z] * cs
        for t in range(F - 1):
            r = s * (F - 1) + t
            h = xin
            for fc, bn, rstd in zip(FC[:2], BN, rs):
                v = ops.matvec(h, p[fc + "/weights"], p[fc + "/biases"])
                h = ops.elu(((v - p[bn + "/moving_mean"]) * rstd) * p[bn + "/gamma"] + p[bn + "/beta"])
            y = ops.matvec(h, p[FC[2] + "/weights"], p[FC[2] + "/biases"])
            pred = y * os_ + xin[:z] * cs
            gt = y_test[r] * os_ + x_test[r, :z] * cs
            pred[z - pn:] = gt[z - pn:]
            z_out[s, t + 1] = pred
            nxt = x_test[r + 1, z:] if t < F - 2 else xin[z:]
            xin = np.concatenate([pred / cs, nxt])
    return z_out


def z_gt(x_test, y_test, S, F, z, code_std, out_std):
    """the ground-truth codes of test_nn, arithmetic on the data alone: [S,F,z] (fp32, the order of the rollout)"""
    x_test, y_test = np.asarray(x_test, F32), np.asarray(y_test, F32)
    cs, os_ = F32(code_std), F32(out_std)
    out = np.zeros((S, F, z), F32)
    for s in range(S):
        r0 = s * (F - 1)
        out[s, 0] = x_test[r0, :z] * cs
        out[s, 1:] = y_test[r0:r0 + F - 1] * os_ + x_test[r0:r0 + F - 1, :z] * cs
    return out


def nn_arrays(code, w_num):
    """data_nn.py:62-113 on the arrays of a code<z>.npz (fp32): the attributes of the reference's BatchManager by name"""
    x, y, p = (np.array(code[k], F32) for k in ("x", "y", "p"))
    s, f = int(code["s"]), int(code["f"])
    o = {"code_std": np.std(x)}
    y = y - x
    o["out_std"] = np.std(y); o["p_std"] = np.std(p)
    x = x / o["code_std"]; y = y / o["out_std"]; p = p / o["p_std"]
    xt = np.concatenate((x, p), axis=-1)
    n_train_s = int(s * 0.95)
    n_train = n_train_s * (f - 1)
    o["x_train"], o["y_train"], o["x_test"], o["y_test"] = xt[:n_train], y[:n_train], xt[n_train:], y[n_train:]
    for tag, ns in (("train", n_train_s), ("test", s - n_train_s)):
        xs, ys = o["x_" + tag], o["y_" + tag]
        xw = np.zeros((ns * (f - w_num), w_num, xt.shape[1]), F32); yw = np.zeros((ns * (f - w_num), w_num, y.shape[1]), F32)
        k = 0
        for i in range(ns):
            for j in range(f - w_num):
                idx = i * (f - 1) + j
                xw[k] = xs[idx:idx + w_num]; yw[k] = ys[idx:idx + w_num]
                k += 1
        o["x_%s_w" % tag], o["y_%s_w" % tag] = xw, yw
    o["num_test_scenes"], o["num_frames"] = s - n_train_s, f
    return o
