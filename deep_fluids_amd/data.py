"""Dataset reader for the reference's on-disk format: counterpart of ``data.py::BatchManager``.

On-disk format (written by the reference's ``scene/*.py``, e.g. scene/smoke_pos_size.py:121-126,215-218,230-234):
  <root>/args.txt            "key: value" lines (num_param, p0.., min_/max_/num_<pname>, num_frames, num_dof, path_format ...)
  <root>/v/%d_%d_%d.npz      x: [Y,X,2] | [Z,Y,X,3] float32 velocity, y: [c_num] parameters  (AE sets: y [dof, frames])
  <root>/v_range.txt         two numbers; x is normalised by max(|r0|, |r1|)     (data.py:87-88, 329)
``generate_smoke_dataset`` writes such a directory for the reference's default 2-D smoke scene with this library's own solver,
``generate_smoke3_obs_dataset`` for its 3-D scene with a sphere obstacle (scene/smoke3_obs_buo.py).
Labels are mapped to [-1,1] with min_/max_<pname> (data.py:331-332).

The reference feeds a tf.FIFOQueue from N Python threads that share one RandomState (data.py:116-144) and dequeues
``batch_size`` samples in-graph.  Here N worker threads fill PINNED host batches and a double-buffered queue hands
them to the GPU with an async copy on a side stream, so the H2D transfer (75 MB per 16 samples at cfg3 = 1.2 ms at
63 GB/s) overlaps the ~0.6 s train step.  Sampling is i.i.d. with replacement per sample, as in the reference.
"""
import os
import queue
import threading
from glob import glob

import numpy as np
import torch


def preprocess(file_path, data_type, x_range, y_range):
    """data.py:311-333."""
    with np.load(file_path) as data:
        x = data["x"].astype(np.float32)
        y = data["y"].astype(np.float32)
    if data_type[0] == "d":
        x = x * 2 - 1
    else:
        x = x / x_range
    for i, ri in enumerate(y_range):
        y[i] = (y[i] - ri[0]) / (ri[1] - ri[0]) * 2 - 1
    return x, y


class BatchManager(object):
    def __init__(self, config, device="cuda", prefetch=2):
        self.rng = np.random.RandomState(config.random_seed)        # data.py:18
        self.root = config.data_path
        self.args = {}
        with open(os.path.join(self.root, "args.txt"), "r") as f:   # data.py:22-29
            for line in f:
                if not line.strip():
                    continue
                arg, arg_value = line.rstrip("\n").split(": ")
                self.args[arg] = arg_value
        self.is_3d = config.is_3d
        self.data_type = config.data_type
        pattern = "{}/{}/*".format(self.root, config.data_type[0])
        if "ae" in config.arch:                                      # data.py:32-38: sort by (sim, frame)
            nf = int(self.args["num_frames"])

            def sortf(p):
                n = os.path.basename(p)[:-4].split("_")
                return int(n[0]) * nf + int(n[1]) if len(n) > 1 else int(n[0])      # "%d.npz": one scene (scene/smoke3_rot.py)
            self.paths = sorted(glob(pattern), key=sortf)
        else:
            self.paths = sorted(glob(pattern))
        self.num_samples = len(self.paths)
        assert self.num_samples > 0                                  # data.py:48
        self.batch_size = config.batch_size
        self.epochs_per_step = self.batch_size / float(self.num_samples)
        self.depth = (3 if self.is_3d else 2) if self.data_type == "velocity" else 1
        self.res_x, self.res_y, self.res_z = config.res_x, config.res_y, config.res_z
        self.c_num = int(self.args["num_param"])
        self.feature_dim = ([self.res_z] if self.is_3d else []) + [self.res_y, self.res_x, self.depth]
        if "ae" in config.arch:
            self.dof = int(self.args["num_dof"])
            self.label_dim = [self.dof, int(self.args["num_frames"])]
        else:
            self.label_dim = [self.c_num]
        r = np.loadtxt(os.path.join(self.root, self.data_type[0] + "_range.txt"))
        self.x_range = max(abs(r[0]), abs(r[1]))                     # data.py:87-88
        self.y_range, self.y_num = [], []
        for i in range(self.c_num):                                  # data.py:92-108
            p_name = self.args["p%d" % i]
            self.y_num.append(int(self.args["num_{}".format(p_name)]))
            if "ae" not in config.arch:
                self.y_range.append([float(self.args["min_{}".format(p_name)]), float(self.args["max_{}".format(p_name)])])
        if "ae" in config.arch:
            self.y_range = [[-1, 1] for _ in range(self.label_dim[0])]
        self.num_threads = int(np.amin([getattr(config, "num_worker", 2), os.cpu_count() or 1, self.batch_size]))
        self.device = torch.device(device) if device is not None else None
        self._q = queue.Queue(maxsize=prefetch)
        self._stop = threading.Event()
        self._threads = []
        self._lock = threading.Lock()
        self._copy_stream = None

    # ---- producer side -------------------------------------------------------------------------------------
    def _make_batch(self):
        pin = self.device is not None and self.device.type == "cuda"
        xb = torch.empty([self.batch_size] + self.feature_dim, dtype=torch.float32, pin_memory=pin)
        yb = torch.empty([self.batch_size] + self.label_dim, dtype=torch.float32, pin_memory=pin)
        for i in range(self.batch_size):
            with self._lock:                                          # the reference shares one RandomState unlocked (benign race)
                idx = self.rng.randint(len(self.paths))
            x_, y_ = preprocess(self.paths[idx], self.data_type, self.x_range, self.y_range)
            xb[i].copy_(torch.from_numpy(np.ascontiguousarray(x_)))
            yb[i].copy_(torch.from_numpy(np.ascontiguousarray(y_)))
        return xb, yb

    def _worker(self):
        while not self._stop.is_set():
            item = self._make_batch()
            while not self._stop.is_set():
                try:
                    self._q.put(item, timeout=0.1)
                    break
                except queue.Full:
                    continue

    def start_thread(self, sess=None):
        """data.py:116-159 (``sess`` is accepted for call-site parity and ignored)."""
        if self._threads:
            return
        self._stop.clear()
        self._threads = [threading.Thread(target=self._worker, daemon=True) for _ in range(self.num_threads)]
        for t in self._threads:
            t.start()

    def stop_thread(self):
        self._stop.set()
        for t in self._threads:
            t.join(timeout=5)
        self._threads = []

    def __del__(self):
        try:
            self.stop_thread()
        except Exception:
            pass

    # ---- consumer side -------------------------------------------------------------------------------------
    def batch(self):
        """One normalised batch (x [B,(Z,)Y,X,C], y [B,c_num] | [B,dof,frames]) on the device (data.py:170-171)."""
        if not self._threads:
            self.start_thread()
        xb, yb = self._q.get()
        if self.device is None or self.device.type != "cuda":
            return xb, yb
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream()
        with torch.cuda.stream(self._copy_stream):
            xd = xb.to(self.device, non_blocking=True)
            yd = yb.to(self.device, non_blocking=True)
        torch.cuda.current_stream().wait_stream(self._copy_stream)
        xd.record_stream(torch.cuda.current_stream()); yd.record_stream(torch.cuda.current_stream())
        return xd, yd

    def batch_(self, b_num):
        """Sequential pass over the whole set (data.py:173-184)."""
        assert len(self.paths) % b_num == 0
        x_batch = []
        for i, filepath in enumerate(self.paths):
            x, _ = preprocess(filepath, self.data_type, self.x_range, self.y_range)
            x_batch.append(x)
            if (i + 1) % b_num == 0:
                yield np.array(x_batch), []
                x_batch = []

    # ---- fixed ground-truth samples of the sample sheets (data.py:197-308) ---------------------------------
    def list_from_p(self, p_list):
        """File paths of the samples with parameter indices ``p_list`` (data.py:197-202)."""
        path_format = os.path.join(self.root, self.data_type[0], self.args["path_format"])
        return [path_format % tuple(p) for p in p_list]

    def _random_p(self):
        p = [self.rng.randint(y_max) for y_max in self.y_num]
        z = [(pi / float(self.y_num[i] - 1)) * 2 - 1 for i, pi in enumerate(p)]      # [-1,1]
        return p, z

    def random_list(self, num):
        """``num`` samples at random parameter indices ``p`` (their normalised values ``z = p/(num-1)*2-1``), on the host.
        2-D (data.py:204-229): ``(xs, pis, zis)`` with xs [num,Y,X,3|1] float images in [0,255] -- velocity gets a zero third channel,
        a level set is thresholded at 0.5 first.  3-D (data.py:231-302): a dict with the fields ``x``, labels ``y``, the four
        ``plane_view_np`` images of every field (``xy, zy, xym, zym``) and of its curl (``*_c``), ``p`` and ``z``."""
        from .ops import plane_view_np
        if not self.is_3d:
            xs, pis, zis = [], [], []
            for _ in range(num):
                pi, zi = self._random_p()
                x, _ = preprocess(self.list_from_p([pi])[0], self.data_type, self.x_range, self.y_range)
                x = x.astype(np.float32)          # the reference normalises in place: the sample stays fp32
                if self.data_type[0] == "v":
                    x = np.concatenate((x, np.zeros((self.res_y, self.res_x, 1))), axis=-1)
                elif self.data_type[0] == "l":
                    x[x < (0.5 + 1e-3)] = -1
                    x[x > -1] = 1
                xs.append(np.clip((x + 1) * 127.5, 0, 255))
                pis.append(pi)
                zis.append(zi)
            return np.array(xs), pis, zis
        keys = ("xy", "zy", "xym", "zym")
        sample = {k: [] for k in ("x", "y") + keys + tuple(k + "_c" for k in keys) + ("p", "z")}
        for _ in range(num):
            p, z = self._random_p()
            sample["p"].append(p)
            sample["z"].append(z)
            x, y = preprocess(self.list_from_p([p])[0], self.data_type, self.x_range, self.y_range)
            x = x.astype(np.float32)              # the reference normalises in place: the sample stays fp32
            sample["x"].append(x)
            sample["y"].append(y)
            x_c = _curl_np3(x)
            for k in keys:
                kw = dict(xy_plane=k[0] == "x", project=not k.endswith("m"))
                sample[k].append(plane_view_np(x, **kw))
                sample[k + "_c"].append(plane_view_np(x_c, **kw))
        for k in sample:
            if k not in ("p", "z"):
                sample[k] = np.array(sample[k])
        return sample

    def denorm(self, x=None, y=None):
        """[-1,1] -> original range (data.py:186-195)."""
        if x is not None:
            x *= self.x_range
        if y is not None:
            for i, ri in enumerate(self.y_range):
                y[:, i] = (y[:, i] + 1) * 0.5 * (ri[1] - ri[0]) + ri[0]
        return x, y


class NNBatchManager(object):
    """The reference's ``data_nn.BatchManager`` (data_nn.py:12-160) for ``arch='nn'``: the codes ``<config.code_path>/code<z_num>.npz``
    that ``AETrainer.test_ae`` wrote, normalised and cut into windows exactly as data_nn.py:62-126 does (``code_std``, ``out_std``,
    ``p_std``; the first ``int(s * 0.95)`` scenes train, the rest test; windows of ``w_size`` consecutive rows per scene with the
    reference's own index ``i * (f - 1) + j``, ``j < f - w_size``), all fp32.  ``p_num`` (``dof``) is ``num_dof`` of
    ``<config.data_path>/args.txt``.

    Batches are consecutive slices of ``batch_size`` rows and the remainder is kept, so the last batch of an epoch is short.  The
    reference shuffles the batches through a ``tf.data`` buffer of 50, which cannot be restated: here the ORDER of an epoch's batches is
    a permutation seeded by (``random_seed``, epoch, window or not) -- this project's own -- so ``seek(step)`` puts a resumed run where
    the interrupted one was.  ``batch`` / ``test_batch`` return ``(x, y)`` tensors on ``device``; the test batches come in file order
    and start over after ``init_test_it()`` or at their end."""

    def __init__(self, config, device="cuda"):
        self.root = config.data_path
        self.args = {}
        with open(os.path.join(self.root, "args.txt"), "r") as f:   # data_nn.py:18-25
            for line in f:
                if line.strip():
                    arg, arg_value = line.rstrip("\n").split(": ")
                    self.args[arg] = arg_value
        self.is_3d = config.is_3d
        self.w_num = int(config.w_size)
        self.z_num = int(config.z_num)
        self.dof = self.p_num = int(self.args["num_dof"])
        self.code_path = os.path.join(config.code_path, "code%d.npz" % self.z_num)
        self.batch_size = int(config.batch_size)
        self.seed = int(config.random_seed)
        self.device = torch.device(device)
        with np.load(self.code_path) as code:                         # data_nn.py:62-69
            x, y, p = (np.array(code[k], np.float32) for k in ("x", "y", "p"))
            self.num_scenes, self.num_frames = int(code["s"]), int(code["f"])
        if x.shape[1] != self.z_num or p.shape[1] != self.p_num or self.p_num > self.z_num:
            raise ValueError("%s: codes of %d with %d parameters, the configuration says z_num %d and args.txt num_dof %d" % (
                self.code_path, x.shape[1], p.shape[1], self.z_num, self.p_num))
        if not 1 <= self.w_num < self.num_frames:
            raise ValueError("w_size %d does not fit scenes of %d frames" % (self.w_num, self.num_frames))
        self.code_std = np.std(x)                                     # data_nn.py:71-78
        y -= x
        self.out_std = np.std(y)
        self.p_std = np.std(p)
        x /= self.code_std
        y /= self.out_std
        p /= self.p_std
        self.x_train = np.concatenate((x, p), axis=-1)
        self.y_train = y
        self.num_train_scenes = int(self.num_scenes * 0.95)           # data_nn.py:83-89
        self.num_test_scenes = self.num_scenes - self.num_train_scenes
        self.num_train = self.num_train_scenes * (self.num_frames - 1)
        self.num_test = self.x_train.shape[0] - self.num_train
        self.x_test, self.y_test = self.x_train[self.num_train:], self.y_train[self.num_train:]
        self.x_train, self.y_train = self.x_train[:self.num_train], self.y_train[:self.num_train]
        self.x_train_w, self.y_train_w = self._windows(self.x_train, self.y_train, self.num_train_scenes)      # data_nn.py:91-113
        self.x_test_w, self.y_test_w = self._windows(self.x_test, self.y_test, self.num_test_scenes)
        self.num_train_w, self.num_test_w = self.x_train_w.shape[0], self.x_test_w.shape[0]
        self.num_samples = self.num_train + self.num_test
        if self.num_train_w < 1 or self.num_test_w < 1:
            raise ValueError("%s: %d scenes leave %d training and %d test windows; both must exist" % (
                self.code_path, self.num_scenes, self.num_train_w, self.num_test_w))
        self.train_steps = max(int(self.num_train / self.batch_size + 0.5), 1)          # data_nn.py:121-126
        self.test_steps = max(int(self.num_test / self.batch_size + 0.5), 1)
        self.train_w_steps = max(int(self.num_train_w / self.batch_size + 0.5), 1)
        self.test_w_steps = max(int(self.num_test_w / self.batch_size + 0.5), 1)
        self.epochs_per_step = 1 / self.train_w_steps
        self.c_num = 0
        self._count = {False: 0, True: 0}
        self._test_at = {False: 0, True: 0}
        self._dev = {}

    def _windows(self, xs, ys, num_scenes):
        n = num_scenes * (self.num_frames - self.w_num)
        xw = np.zeros([n, self.w_num, xs.shape[1]], np.float32)
        yw = np.zeros([n, self.w_num, ys.shape[1]], np.float32)
        k = 0
        for i in range(num_scenes):
            for j in range(self.num_frames - self.w_num):
                idx = i * (self.num_frames - 1) + j
                xw[k], yw[k] = xs[idx:idx + self.w_num], ys[idx:idx + self.w_num]
                k += 1
        return xw, yw

    def _on_device(self, name):
        if name not in self._dev:
            self._dev[name] = torch.from_numpy(np.ascontiguousarray(getattr(self, name), np.float32)).to(self.device)
        return self._dev[name]

    def _slice(self, tag, is_window, b):
        sfx = "_w" if is_window else ""
        x, y = self._on_device("x_%s%s" % (tag, sfx)), self._on_device("y_%s%s" % (tag, sfx))
        return x[b * self.batch_size:(b + 1) * self.batch_size].contiguous(), y[b * self.batch_size:(b + 1) * self.batch_size].contiguous()

    def num_batches(self, is_window=False, test=False):
        """batches per pass over the set, the short last one included"""
        n = {(False, False): self.num_train, (True, False): self.num_train_w, (False, True): self.num_test, (True, True): self.num_test_w}[
            (bool(is_window), bool(test))]
        return -(-n // self.batch_size)

    def batch_index(self, count, is_window=False):
        """which batch of the training set the ``count``-th call of ``batch`` returns"""
        nb = self.num_batches(is_window)
        order = np.random.RandomState([self.seed, count // nb, int(bool(is_window))]).permutation(nb)
        return int(order[count % nb])

    def seek(self, count, is_window=False):
        self._count[bool(is_window)] = int(count)

    def batch(self, is_window=False):
        w = bool(is_window)
        b = self.batch_index(self._count[w], w)
        self._count[w] += 1
        return self._slice("train", w, b)

    def init_test_it(self):
        self._test_at = {False: 0, True: 0}

    def test_batch(self, is_window=False):
        w = bool(is_window)
        b = self._test_at[w]
        self._test_at[w] = (b + 1) % self.num_batches(w, test=True)
        return self._slice("test", w, b)


def _curl_np3(x):
    """Host NumPy curl of x [Z,Y,X,3] -- the ``c`` of ``jacobian_np3`` (ops.py:344-374): forward differences with the last difference
    replicated, c = (dwdy - dvdz, dudz - dwdx, dvdx - dudy).  On the host because ``random_list`` runs once, on ``b_num`` samples."""
    def d(a, axis):
        g = np.diff(a, axis=axis)
        return np.concatenate([g, np.take(g, [-1], axis=axis)], axis=axis)
    u, v, w = x[..., 0], x[..., 1], x[..., 2]
    return np.stack([d(w, 1) - d(v, 0), d(u, 0) - d(w, 2), d(v, 2) - d(u, 1)], axis=-1)


def write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=4, seed=0, ae=False):
    """Write a tiny dataset in the reference's on-disk format (tests / demos; there is no network for real data)."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "v"), exist_ok=True)
    is_3d = len(spatial) == 3
    lines = ["num_param: 3", "p0: src_x_pos", "p1: src_radius", "p2: frames",
             "min_src_x_pos: 0.2", "max_src_x_pos: 0.8", "num_src_x_pos: %d" % num_p[0],
             "min_src_radius: 0.04", "max_src_radius: 0.12", "num_src_radius: %d" % num_p[1],
             "min_frames: 0", "max_frames: %d" % (num_frames - 1), "num_frames: %d" % num_frames,
             "num_dof: 2", "path_format: %d_%d_%d.npz"]
    with open(os.path.join(root, "args.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    vmax = 0.0
    for i in range(num_p[0]):
        for j in range(num_p[1]):
            for t in range(num_frames):
                x = rng.uniform(-2, 2, size=list(spatial) + [3 if is_3d else 2]).astype(np.float32)
                vmax = max(vmax, float(np.abs(x).max()))
                px = 0.2 + 0.6 * i / max(num_p[0] - 1, 1); pr = 0.04 + 0.08 * j / max(num_p[1] - 1, 1)
                y = rng.uniform(-1, 1, size=(2, num_frames)).astype(np.float32) if ae else np.array([px, pr, t], np.float32)
                np.savez_compressed(os.path.join(root, "v", "%d_%d_%d.npz" % (i, j, t)), x=x, y=y)
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n%.3f\n" % (-vmax, vmax))
    return num_p[0] * num_p[1] * num_frames


def write_synthetic_ae_dataset(root, spatial, num_scenes=2, num_frames=4, seed=0):
    """A tiny dataset in the on-disk format of the reference's moving-source scenes (scene/smoke3_mov.py:18-38,176-182,286-326 --
    what ``--arch=ae`` trains on, run.bat:56,73): ``v/<scene>_<frame>.npz`` with x = velocity [(Z,)Y,X,2|3] and y = source positions
    [dof, frames]; ``n.npz`` with the noise tracks ``nx`` (and ``nz`` in 3-D) [scenes, frames]; ``args.txt``; ``v_range.txt``."""
    rng = np.random.RandomState(seed)
    os.makedirs(os.path.join(root, "v"), exist_ok=True)
    is_3d = len(spatial) == 3
    dof = 2 if is_3d else 1
    lines = ["num_param: 2", "path_format: %d_%d.npz", "p0: scenes", "p1: frames", "min_scenes: 0", "max_scenes: %d" % (num_scenes - 1),
             "num_scenes: %d" % num_scenes, "min_frames: 0", "max_frames: %d" % (num_frames - 1), "num_frames: %d" % num_frames,
             "num_simulations: %d" % (num_scenes * num_frames), "num_dof: %d" % dof]
    with open(os.path.join(root, "args.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    nx = rng.uniform(-1, 1, (num_scenes, num_frames)).astype(np.float32)
    nz = rng.uniform(-1, 1, (num_scenes, num_frames)).astype(np.float32)
    vmax = 0.0
    for i in range(num_scenes):
        for t in range(num_frames):
            x = rng.uniform(-2, 2, size=list(spatial) + [3 if is_3d else 2]).astype(np.float32)
            vmax = max(vmax, float(np.abs(x).max()))
            y = np.stack([nx[i], nz[i]])[:dof].astype(np.float32)           # [dof, frames]; the trainer reads y[:, :, -1]
            np.savez_compressed(os.path.join(root, "v", "%d_%d.npz" % (i, t)), x=x, y=y)
    if is_3d:
        np.savez_compressed(os.path.join(root, "n.npz"), nx=nx, nz=nz)
    else:
        np.savez_compressed(os.path.join(root, "n.npz"), nx=nx)
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n%.3f\n" % (-vmax, vmax))
    return num_scenes * num_frames


def generate_smoke_dataset(root, num_param=3, path_format="%d_%d_%d.npz", p0="src_x_pos", p1="src_radius", p2="frames", num_src_x_pos=21,
                           min_src_x_pos=0.2, max_src_x_pos=0.8, src_y_pos=0.1, num_src_radius=5, min_src_radius=0.04, max_src_radius=0.12,
                           num_frames=200, min_frames=0, max_frames=None, num_simulations=None, resolution_x=96, resolution_y=128,
                           buoyancy=-4e-3, bWidth=1, open_bound=False, time_step=0.5, adv_order=2, clamp_mode=2, scenes_per_batch=None,
                           accuracy=1e-4, device="cuda", preconditioner=None):
    """Simulate the reference's default 2-D training set (scene/smoke_pos_size.py:111-254, ``smoke_pos21_size5_f200``) on the GPU and
    write it in the reference's on-disk format: ``args.txt`` with every argument of the scene script, ``v/%d_%d_%d.npz`` (x [Y,X,2]
    float32 velocity after frame t, y = [p0, p1, t]) and ``v_range.txt``.  The keyword arguments are the script's, with its defaults.
    Every scene is one batch entry of ``ops.simulate_smoke`` (``scenes_per_batch`` splits the set into chunks; an entry's result does
    not depend on the rest of its batch).  The step is this library's restatement (include/deepfluids_hip.h), not mantaflow's: plain CG
    in place of MIC(0)-preconditioned CG (``preconditioner="mg"``: multigrid-preconditioned, see ``ops.solve_pressure``; the files and
    the ``args.txt`` keys are the same).  ``open_bound``: a string of the open sides, ``'xXyY'`` being what the script's
    ``--open_bound True`` opens, simulated with this library's open-side rules and zero-gradient fill (tests/smoke_open_ref.py), not
    mantaflow's outflow.  The bare ``True`` is still refused: it would promise the script's mantaflow outflow, which is not restated;
    name the sides.  Returns the number of files written."""
    from . import ops
    if open_bound is True:
        raise NotImplementedError("generate_smoke_dataset: open_bound=True (mantaflow's outflow) is not restated; pass the open sides as "
                                  "a string, 'xXyY' for the script's, to simulate them with this library's open-side rules")
    sides = ops.open_sides(open_bound, 2)
    if num_param != 3 or (p0, p1, p2) != ("src_x_pos", "src_radius", "frames"):
        raise ValueError("generate_smoke_dataset: the scene has the parameters (src_x_pos, src_radius, frames)")
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_src_x_pos * num_src_radius * num_frames if num_simulations is None else num_simulations
    args = [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1), ("p2", p2),
            ("num_src_x_pos", num_src_x_pos), ("min_src_x_pos", min_src_x_pos), ("max_src_x_pos", max_src_x_pos), ("src_y_pos", src_y_pos),
            ("num_src_radius", num_src_radius), ("min_src_radius", min_src_radius), ("max_src_radius", max_src_radius),
            ("num_frames", num_frames), ("min_frames", min_frames), ("max_frames", max_frames), ("num_simulations", num_simulations),
            ("resolution_x", resolution_x), ("resolution_y", resolution_y), ("buoyancy", buoyancy), ("bWidth", bWidth),
            ("open_bound", open_bound), ("time_step", time_step), ("adv_order", adv_order), ("clamp_mode", clamp_mode)]
    os.makedirs(os.path.join(root, "v"), exist_ok=True)
    with open(os.path.join(root, "args.txt"), "w") as f:
        for k, v in args:
            f.write("%s: %s\n" % (k, v))

    def param(i, num, lo, hi):                       # get_param of the scene script (what trainer.smoke_pos_size_source evaluates)
        return i / float(num - 1) * (hi - lo) + lo if num > 1 else lo

    scenes = [(i, j, param(i, num_src_x_pos, min_src_x_pos, max_src_x_pos), param(j, num_src_radius, min_src_radius, max_src_radius))
              for i in range(num_src_x_pos) for j in range(num_src_radius)]
    X, Y = int(resolution_x), int(resolution_y)
    chunk = len(scenes) if not scenes_per_batch else int(scenes_per_batch)
    force = ops.default_buoyancy_force((Y, X), time_step, gravity=buoyancy)
    v_range = [np.finfo(np.float64).max, np.finfo(np.float64).min]
    written = 0
    for c0 in range(0, len(scenes), chunk):
        part = scenes[c0:c0 + chunk]
        mask = torch.stack([ops.sphere_mask((Y, X), (X * px, Y * src_y_pos), X * pr) for _, _, px, pr in part]).to(device)
        d0 = torch.zeros((len(part), Y, X), dtype=torch.float32, device=device)
        v0 = torch.zeros((len(part), Y, X, 2), dtype=torch.float32, device=device)
        frames = ops.simulate_smoke(d0, v0, num_frames, dt=time_step, source=mask, force=force, order=adv_order, clamp_mode=clamp_mode,
                                    bnd=bWidth, accuracy=accuracy, stack=False, open_bound=sides, preconditioner=preconditioner)
        for t, (_, v) in enumerate(frames):
            vh = v.cpu().numpy()
            v_range = [min(v_range[0], float(vh.min())), max(v_range[1], float(vh.max()))]
            for e, (i, j, px, pr) in enumerate(part):
                np.savez_compressed(os.path.join(root, "v", path_format % (i, j, t)), x=vh[e], y=[px, pr, t])
                written += 1
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n" % v_range[0])
        f.write("%.3f" % v_range[1])
    return written


def _simulate_liquid_scenes(root, path_format, scenes, shape, num_frames, time_step, gravity, bWidth, accuracy, flip_ratio, device, keep,
                            alphas=None, substeps=1, label=None, ghost_fluid=False, radius_factor=1.0, resample=None, preconditioner=None):
    """the frame loop of the liquid scene scripts: ``scenes`` = (i, j, p0, p1, phi0, velocity spheres); scenes that seed the same number
    of particles run as one batch of ``ops.simulate_liquid``.  Writes v/ and v_range.txt; returns the number of files written.
    ``alphas``: one diffusion number per scene (the viscous step); ``substeps``: solver steps per frame, frame f is step f * substeps;
    ``label(scene, frame)``: the numbers of a file's name and its ``y``; ``ghost_fluid``: every step builds the averaged level set
    (``radius_factor``) and projects against the ghost-fluid surface (``ops.liquid_step``).  ``resample``: None, or ``min_particles``: the
    steps run extrapolateLsSimple and adjustNumber on a ragged batch, and ALL scenes, whatever they seed, share one batch.
    ``preconditioner``: None or an ``ops.Multigrid``, handed to ``ops.simulate_liquid``."""
    from . import ops
    if label is None:
        def label(sc, t):
            return (sc[0], sc[1], t), [sc[2], sc[3], t]
    states = [ops.liquid_initial_state(shape, phi, spheres, bnd=bWidth, device=device) for _, _, _, _, phi, spheres in scenes]
    groups = {}
    for n, st in enumerate(states):
        groups.setdefault(int(st[0].shape[1]), []).append(n)
    force = ops.default_gravity_force(shape, time_step, gravity=gravity)
    v_range = [np.finfo(np.float64).max, np.finfo(np.float64).min]
    written = 0
    if resample is not None:
        groups = {0: list(range(len(states)))}
    for N in sorted(groups):
        part = groups[N]
        if resample is None:
            pos, pvel, vel = [torch.cat([states[n][k] for n in part]) for k in range(3)]
        else:
            total = sum(int(states[n][0].shape[1]) for n in part)
            cap = -(-2 * total // len(part)) * len(part)
            pos, es = ops.pack_particles([states[n][0][0] for n in part], capacity=cap)
            pvel, _ = ops.pack_particles([states[n][1][0] for n in part], capacity=cap)
            vel = torch.cat([states[n][2] for n in part])
        more = {} if alphas is None and substeps == 1 else dict(viscosity_alpha=None if alphas is None else [alphas[n] for n in part],
                                                                keep_every=substeps)
        if ghost_fluid:
            more.update(ghost_fluid=True, radius_factor=float(radius_factor))
        if resample is not None:
            more.update(resample=ops.Resample(int(resample)), entry_start=es, radius_factor=float(radius_factor))
        if preconditioner is not None:
            more.update(preconditioner=preconditioner)
        frames = ops.simulate_liquid(pos, pvel, vel, (num_frames - 1) * substeps + 1 if num_frames > 0 else 0, dt=time_step, force=force,
                                     bnd=bWidth, accuracy=accuracy, flip_ratio=flip_ratio, stack=False, **more)
        for t, frame in enumerate(frames):
            vh = frame[2].cpu().numpy()
            v_range = [min(v_range[0], float(vh.min())), max(v_range[1], float(vh.max()))]
            for e, n in enumerate(part):
                name, y = label(scenes[n], t)
                np.savez_compressed(os.path.join(root, "v", path_format % name), x=vh[e][..., :keep], y=y)
                written += 1
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n" % v_range[0])
        f.write("%.3f" % v_range[1])
    return written


def _write_args(root, args):
    os.makedirs(os.path.join(root, "v"), exist_ok=True)
    with open(os.path.join(root, "args.txt"), "w") as f:
        for k, v in args:
            f.write("%s: %s\n" % (k, v))


def _liquid_refusals(who, open_bound, num_param, names, want):
    if open_bound:
        raise NotImplementedError("%s: open_bound (setOpenBound + resetOutflow) is not implemented for the liquid solver" % who)
    if num_param != len(want) or tuple(names) != tuple(want):
        raise ValueError("%s: the scene has the parameters %s" % (who, (want,)))


def generate_liquid_dataset(root, num_param=3, path_format="%d_%d_%d.npz", p0="src_x_pos", p1="src_radius", p2="frames", num_src_x_pos=10,
                            min_src_x_pos=0.2, max_src_x_pos=0.8, src_y_pos=0.6, num_src_radius=4, min_src_radius=0.04, max_src_radius=0.08,
                            basin_y_pos=0.2, num_frames=200, min_frames=0, max_frames=None, num_simulations=None, resolution_x=128,
                            resolution_y=64, gravity=-1e-3, radius_factor=1, min_particles=2, bWidth=1, open_bound=False, time_step=0.5,
                            accuracy=1e-4, flip_ratio=0.97, device="cuda", ghost_fluid=False, resample=False, preconditioner=None):
    """Simulate the reference's 2-D liquid training set (scene/liquid_pos_size.py:148-325, ``liquid_pos10_size4_f200``) on the GPU and
    write it in the reference's on-disk format: ``args.txt`` with every argument of the scene script, ``v/%d_%d_%d.npz`` (x [Y,X,2]
    float32 velocity after frame t, y = [p0, p1, t]) and ``v_range.txt``.  The keyword arguments are the script's, with its defaults
    (``min_particles`` is recorded only unless ``resample=True``, which runs the script's extrapolateLsSimple + adjustNumber(minParticles,
    2 * minParticles) in every step on ONE ragged batch of all scenes, with the same files and ``args.txt`` keys; ``radius_factor`` is recorded, and used by ``ghost_fluid=True``
    alone).  A drop of radius p1 at
    (p0, src_y_pos) falls into a basin of height basin_y_pos; scenes that seed the same number of particles run as one batch of
    ``ops.simulate_liquid``.  The step is this library's restatement (include/deepfluids_hip.h), not mantaflow's: by default a
    first-order free surface (p = 0 at the air cell centres) and plain CG; with ``ghost_fluid=True`` (not a script argument: the same
    files, the same ``args.txt`` keys) every step builds the averaged level set of ``radius_factor`` and projects against the
    ghost-fluid surface with preconditioned CG, as the script's loop does (``ops.liquid_step``).  ``open_bound=True`` is refused.
    ``preconditioner=ops.Multigrid(...)`` (not a script argument either: the same files, the same ``args.txt`` keys): the projections are
    multigrid-preconditioned (``ops.liquid_step``).  Returns the number of files written."""
    from . import ops
    _liquid_refusals("generate_liquid_dataset", open_bound, num_param, (p0, p1, p2), ("src_x_pos", "src_radius", "frames"))
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_src_x_pos * num_src_radius * num_frames if num_simulations is None else num_simulations
    _write_args(root, [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1), ("p2", p2),
                       ("num_src_x_pos", num_src_x_pos), ("min_src_x_pos", min_src_x_pos), ("max_src_x_pos", max_src_x_pos),
                       ("src_y_pos", src_y_pos), ("num_src_radius", num_src_radius), ("min_src_radius", min_src_radius),
                       ("max_src_radius", max_src_radius), ("basin_y_pos", basin_y_pos), ("num_frames", num_frames),
                       ("min_frames", min_frames), ("max_frames", max_frames), ("num_simulations", num_simulations),
                       ("resolution_x", resolution_x), ("resolution_y", resolution_y), ("gravity", gravity), ("radius_factor", radius_factor),
                       ("min_particles", min_particles), ("bWidth", bWidth), ("open_bound", open_bound), ("time_step", time_step)])

    def param(i, num, lo, hi):
        return i / float(num - 1) * (hi - lo) + lo if num > 1 else lo

    X, Y = int(resolution_x), int(resolution_y)
    basin = ops.box_levelset((Y, X), (0.0, 0.0), (X * 1.0, Y * basin_y_pos))
    scenes = []
    for i in range(num_src_x_pos):
        for j in range(num_src_radius):
            px, pr = param(i, num_src_x_pos, min_src_x_pos, max_src_x_pos), param(j, num_src_radius, min_src_radius, max_src_radius)
            c = (X * px, Y * src_y_pos)
            phi = np.minimum(basin, ops.sphere_levelset((Y, X), c, X * pr))
            scenes.append((i, j, px, pr, phi, [(c, X * (pr + 0.05))]))
    return _simulate_liquid_scenes(root, path_format, scenes, (Y, X), num_frames, time_step, gravity, bWidth, accuracy, flip_ratio, device, 2,
                                   ghost_fluid=ghost_fluid, radius_factor=radius_factor, resample=min_particles if resample else None,
                                   preconditioner=preconditioner)


def generate_liquid3_d_r_dataset(root, num_param=3, path_format="%d_%d_%d.npz", p0="dist", p1="rot", p2="frames", min_dist=0.15, max_dist=0.25,
                                 num_dist=5, min_rot=0, max_rot=162, num_rot=10, src_y_pos=0.6, src_radius=0.1, basin_y_pos=0.2,
                                 min_frames=0, max_frames=None, num_frames=150, num_simulations=None, resolution_x=96, resolution_y=48,
                                 resolution_z=96, gravity=-1e-3, radius_factor=1, min_particles=3, bWidth=1, open_bound=False,
                                 time_step=0.8, accuracy=1e-4, flip_ratio=0.97, device="cuda", ghost_fluid=False, resample=False, preconditioner=None):
    """Simulate the reference's 3-D liquid training set (scene/liquid3_d_r.py main(), ``liquid3_d5_r10_f150``) on the GPU, in the same
    on-disk format (x [Z,Y,X,3]): two drops of radius src_radius at distance p0 (fractions of X) either side of the centre, the pair
    rotated by p1 degrees about the vertical axis, fall into a basin.  The keyword arguments are the script's, with its defaults; what
    ``generate_liquid_dataset`` says about the step, about ``ghost_fluid`` (which alone uses ``radius_factor``), about ``preconditioner`` and about what
    is left out holds here too."""
    from . import ops
    _liquid_refusals("generate_liquid3_d_r_dataset", open_bound, num_param, (p0, p1, p2), ("dist", "rot", "frames"))
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_dist * num_rot * num_frames if num_simulations is None else num_simulations
    _write_args(root, [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1), ("p2", p2),
                       ("min_dist", min_dist), ("max_dist", max_dist), ("num_dist", num_dist), ("min_rot", min_rot), ("max_rot", max_rot),
                       ("num_rot", num_rot), ("src_y_pos", src_y_pos), ("src_radius", src_radius), ("basin_y_pos", basin_y_pos),
                       ("min_frames", min_frames), ("max_frames", max_frames), ("num_frames", num_frames),
                       ("num_simulations", num_simulations), ("resolution_x", resolution_x), ("resolution_y", resolution_y),
                       ("resolution_z", resolution_z), ("gravity", gravity), ("radius_factor", radius_factor),
                       ("min_particles", min_particles), ("bWidth", bWidth), ("open_bound", open_bound), ("time_step", time_step)])
    X, Y, Z = int(resolution_x), int(resolution_y), int(resolution_z)
    shape = (Z, Y, X)
    basin = ops.box_levelset(shape, (0.0, 0.0, 0.0), (X * 1.0, Y * basin_y_pos, Z * 1.0))
    centre = (X * 0.5, Y * src_y_pos, Z * 0.5)
    scenes = []
    for i, dist in enumerate(np.linspace(min_dist, max_dist, num_dist)):
        for j, rot in enumerate(np.linspace(min_rot, max_rot, num_rot)):
            r, th = X * dist, rot / 180.0 * np.pi
            cs = [(centre[0] + r * np.cos(t), centre[1], centre[2] + r * np.sin(t)) for t in (th, th + np.pi)]
            phi = basin
            for c in cs:
                phi = np.minimum(phi, ops.sphere_levelset(shape, c, X * src_radius))
            scenes.append((i, j, float(dist), float(rot), phi, [(c, X * (src_radius + 0.05)) for c in cs]))
    return _simulate_liquid_scenes(root, path_format, scenes, shape, num_frames, time_step, gravity, bWidth, accuracy, flip_ratio, device, 3,
                                   ghost_fluid=ghost_fluid, radius_factor=radius_factor, resample=min_particles if resample else None,
                                   preconditioner=preconditioner)


def generate_liquid3_vis_dataset(root, num_param=2, path_format="%d_%d.npz", p0="viscosity", p1="frames", viscosity_base=2, vmin=-5, vmax=-2,
                                 min_viscosity=0, max_viscosity=3, num_viscosity=4, src_x_pos=0.4, src_y_pos=0.8, src_z_pos=0.4,
                                 min_frames=0, max_frames=None, num_frames=150, num_simulations=None, resolution_x=96, resolution_y=72,
                                 resolution_z=48, gravity=-1e-3, radius_factor=1, min_particles=3, bWidth=1, open_bound=False,
                                 time_step=0.125, accuracy=1e-4, flip_ratio=0.97, device="cuda", ghost_fluid=False, resample=False, preconditioner=None):
    """Simulate the reference's viscous 3-D liquid training set (scene/liquid3_vis.py main(), ``liquid3_vis4_f150``) on the GPU, in the
    on-disk format of the script: ``args.txt`` with every script argument, ``v/%d_%d.npz`` (x [Z,Y,X,3] float32 velocity of frame f,
    y = [p, f]) and ``v_range.txt``.  The box 0.3..0.7 x 0..0.8 x 0.3..0.7 of the grid (``trainer.liquid3_vis_body``) collapses from rest
    under gravity at ``num_viscosity`` viscosities ``vis_list[int(p)]``, ``p`` the parameter values
    ``linspace(min_viscosity, max_viscosity, num_viscosity)`` and ``vis_list = viscosity_base * logspace(vmin, vmax, num_viscosity)``.  Every
    solver step diffuses the velocity implicitly (``ops.diffuse_velocity``) with ``alpha = ops.diffusion_alpha(visc, time_step,
    resolution_x)``; a frame is ``round(1 / time_step)`` steps, frame f is saved after step ``f * substeps`` (the script's
    ``timeTotal.is_integer()``), and a ``time_step`` whose reciprocal is not an integer is refused.  All scenes seed the same particles
    and run as ONE batch.  ``src_*_pos`` and ``min_particles`` are recorded only (the script does not use the first three either;
    adjustNumber runs with ``resample=True`` alone, as in ``generate_liquid_dataset``); ``radius_factor`` is recorded, and used by ``ghost_fluid=True`` alone.  What ``generate_liquid_dataset``
    says about the step, about ``ghost_fluid`` and about ``preconditioner`` (which, with ``Multigrid.diffusion``, serves the diffusion
    solves too) holds here too.  With ``Multigrid.diffusion`` the frames of the viscous scenes differ from the plain arm's by far more
    than ``accuracy``: at this scene's larger alphas the plain diffusion stops at its iteration cap (``max(extent)`` = 96) short of the
    accuracy and the preconditioned one converges (``ops.liquid_step``); ``Multigrid(diffusion=False)`` keeps the plain diffusion.
    ``open_bound=True`` is refused.  Returns the number of files written."""
    from . import ops
    _liquid_refusals("generate_liquid3_vis_dataset", open_bound, num_param, (p0, p1), ("viscosity", "frames"))
    steps_per_frame = 1.0 / float(time_step) if time_step > 0 else 0.0
    substeps = int(round(steps_per_frame))
    if substeps < 1 or abs(steps_per_frame - substeps) > 1e-9 * substeps:
        raise ValueError("generate_liquid3_vis_dataset: 1 / time_step must be a whole number of steps per frame, got time_step = %r" % (time_step,))
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_viscosity * num_frames if num_simulations is None else num_simulations
    p_list = np.linspace(min_viscosity, max_viscosity, num_viscosity)
    vis_list = viscosity_base * np.logspace(vmin, vmax, num_viscosity)
    if any(not 0 <= int(p) < num_viscosity for p in p_list):
        raise ValueError("generate_liquid3_vis_dataset: the parameter values %s do not index the %d viscosities" % (p_list.tolist(), num_viscosity))
    _write_args(root, [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1),
                       ("viscosity_base", viscosity_base), ("vmin", vmin), ("vmax", vmax), ("min_viscosity", min_viscosity),
                       ("max_viscosity", max_viscosity), ("num_viscosity", num_viscosity), ("src_x_pos", src_x_pos), ("src_y_pos", src_y_pos),
                       ("src_z_pos", src_z_pos), ("min_frames", min_frames), ("max_frames", max_frames), ("num_frames", num_frames),
                       ("num_simulations", num_simulations), ("resolution_x", resolution_x), ("resolution_y", resolution_y),
                       ("resolution_z", resolution_z), ("gravity", gravity), ("radius_factor", radius_factor),
                       ("min_particles", min_particles), ("bWidth", bWidth), ("open_bound", open_bound), ("time_step", time_step)])
    X, Y, Z = int(resolution_x), int(resolution_y), int(resolution_z)
    shape = (Z, Y, X)
    phi = ops.box_levelset(shape, (X * 0.3, 0.0, Z * 0.3), (X * 0.7, Y * 0.8, Z * 0.7))
    scenes = [(i, None, float(p), None, phi, []) for i, p in enumerate(p_list)]
    alphas = [ops.diffusion_alpha(float(vis_list[int(p)]), float(time_step), X) for p in p_list]
    return _simulate_liquid_scenes(root, path_format, scenes, shape, num_frames, time_step, gravity, bWidth, accuracy, flip_ratio, device, 3,
                                   alphas=alphas, substeps=substeps, label=lambda sc, f: ((sc[0], f), [sc[2], f]), ghost_fluid=ghost_fluid, resample=min_particles if resample else None,
                                   radius_factor=radius_factor, preconditioner=preconditioner)


def generate_smoke3_obs_dataset(root, num_param=3, path_format="%d_%d_%d.npz", p0="obs_x_pos", p1="buoyancy", p2="frames", min_obs_x_pos=0.2,
                                max_obs_x_pos=0.8, num_obs_x_pos=11, obs_radius=0.15, obs_y_pos=0.5, obs_z_pos=0.5, min_buoyancy=-8e-3,
                                max_buoyancy=-16e-3, num_buoyancy=4, src_x_pos=0.5, src_y_pos=0.13, src_z_pos=0.5, src_radius=0.12,
                                min_frames=0, max_frames=None, num_frames=150, num_simulations=None, resolution_x=64, resolution_y=96,
                                resolution_z=64, bWidth=1, open_bound=False, time_step=0.5, adv_order=2, clamp_mode=2, scenes_per_batch=None,
                                accuracy=1e-4, device="cuda", preconditioner=None):
    """Simulate the reference's 3-D obstacle training set (scene/smoke3_obs_buo.py:126-294, ``smoke3_obs11_buo4_f150``) on the GPU and
    write it in the reference's on-disk format: ``args.txt`` with every argument of the scene script, ``v/%d_%d_%d.npz`` (x [Z,Y,X,3]
    float32 velocity after frame t, y = [p0, p1, t]) and ``v_range.txt``.  The keyword arguments are the script's, with its defaults
    (``max_frames`` and ``num_simulations`` follow ``num_frames`` and the grid of scenes unless given).  A closed box with a sphere
    source at ``gs * (src_x_pos, src_y_pos, src_z_pos)`` of radius ``X * src_radius`` and a sphere obstacle at ``gs * (p0, obs_y_pos,
    obs_z_pos)`` of radius ``X * obs_radius``; the buoyancy is (0, p1, 0).  Every scene is one batch entry of ``ops.simulate_smoke``.
    The buoyancy is one number per launch, so a chunk holds the scenes of ONE buoyancy value (all obstacle positions: 11 by default);
    ``scenes_per_batch`` splits a chunk further, and an entry's result does not depend on the rest of its batch.  The step is this
    library's restatement (include/deepfluids_hip.h), not mantaflow's: plain CG in place of MIC(0)-preconditioned CG.  The script hands
    ``open_bound`` to advectSemiLagrange only and never calls setOpenBound, so its ``True`` names no sides and is still refused; a
    string of ``xXyYzZ`` opens those sides with this library's open-side rules (tests/smoke_open_ref.py).  Returns the number of files
    written."""
    from . import ops
    if open_bound is True:
        raise NotImplementedError("generate_smoke3_obs_dataset: open_bound=True names no sides (the script never calls setOpenBound); pass "
                                  "the open sides as a string of xXyYzZ")
    sides = ops.open_sides(open_bound, 3)
    if num_param != 3 or (p0, p1, p2) != ("obs_x_pos", "buoyancy", "frames"):
        raise ValueError("generate_smoke3_obs_dataset: the scene has the parameters (obs_x_pos, buoyancy, frames)")
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_obs_x_pos * num_buoyancy * num_frames if num_simulations is None else num_simulations
    args = [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1), ("p2", p2),
            ("min_obs_x_pos", min_obs_x_pos), ("max_obs_x_pos", max_obs_x_pos), ("num_obs_x_pos", num_obs_x_pos), ("obs_radius", obs_radius),
            ("obs_y_pos", obs_y_pos), ("obs_z_pos", obs_z_pos), ("min_buoyancy", min_buoyancy), ("max_buoyancy", max_buoyancy),
            ("num_buoyancy", num_buoyancy), ("src_x_pos", src_x_pos), ("src_y_pos", src_y_pos), ("src_z_pos", src_z_pos),
            ("src_radius", src_radius), ("min_frames", min_frames), ("max_frames", max_frames), ("num_frames", num_frames),
            ("num_simulations", num_simulations), ("resolution_x", resolution_x), ("resolution_y", resolution_y),
            ("resolution_z", resolution_z), ("bWidth", bWidth), ("open_bound", open_bound), ("time_step", time_step),
            ("adv_order", adv_order), ("clamp_mode", clamp_mode)]
    os.makedirs(os.path.join(root, "v"), exist_ok=True)
    with open(os.path.join(root, "args.txt"), "w") as f:
        for k, v in args:
            f.write("%s: %s\n" % (k, v))
    X, Y, Z = int(resolution_x), int(resolution_y), int(resolution_z)
    shape = (Z, Y, X)
    xs = np.linspace(min_obs_x_pos, max_obs_x_pos, num_obs_x_pos)            # p1_space / p2_space of the scene script
    bs = np.linspace(min_buoyancy, max_buoyancy, num_buoyancy)
    source = ops.sphere_mask(shape, (X * src_x_pos, Y * src_y_pos, Z * src_z_pos), X * src_radius).to(device)
    chunk = num_obs_x_pos if not scenes_per_batch else int(scenes_per_batch)
    v_range = [np.finfo(np.float64).max, np.finfo(np.float64).min]
    written = 0
    for j, buo in enumerate(bs):
        force = ops.default_buoyancy_force(shape, time_step, gravity=float(buo))
        for c0 in range(0, num_obs_x_pos, chunk):
            part = list(range(c0, min(c0 + chunk, num_obs_x_pos)))
            obs = torch.stack([ops.sphere_mask(shape, (X * xs[i], Y * obs_y_pos, Z * obs_z_pos), X * obs_radius) for i in part]).to(device)
            d0 = torch.zeros((len(part),) + shape, dtype=torch.float32, device=device)
            v0 = torch.zeros((len(part),) + shape + (3,), dtype=torch.float32, device=device)
            frames = ops.simulate_smoke(d0, v0, num_frames, dt=time_step, source=source, force=force, order=adv_order, clamp_mode=clamp_mode,
                                        bnd=bWidth, accuracy=accuracy, stack=False, obstacle=ops.obstacle_flags(obs, bWidth),
                                        open_bound=sides, preconditioner=preconditioner)
            for t, (_, v) in enumerate(frames):
                vh = v.cpu().numpy()
                v_range = [min(v_range[0], float(vh.min())), max(v_range[1], float(vh.max()))]
                for e, i in enumerate(part):
                    np.savez_compressed(os.path.join(root, "v", path_format % (i, j, t)), x=vh[e], y=[xs[i], buo, t])
                    written += 1
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n" % v_range[0])
        f.write("%.3f" % v_range[1])
    return written


# ---- the moving-source scenes (scene/smoke3_rot.py, scene/smoke3_mov.py): open sides, a sphere source whose centre changes every frame ----
def smooth_source_paths(num_scenes, num_frames, lo, hi, seed=123, modes=3):
    """Seeded smooth source paths [num_scenes, num_frames, 2] (x and z as fractions of the grid) inside ``[lo, hi]``: per scene and
    coordinate a sum of ``modes`` sines of random period (100..400 frames), phase and weight, normalised by the sum of the weights.
    This is the project's own stand-in: it is NOT the reference's tileable Perlin noise (scene/perlin.py), only a path of the same
    kind -- smooth, bounded, different per scene and reproducible from the seed."""
    rng = np.random.RandomState(seed)
    t = np.arange(num_frames, dtype=np.float64)
    out = np.empty((num_scenes, num_frames, 2), np.float64)
    for i in range(num_scenes):
        for c in range(2):
            w = rng.uniform(0.4, 1.0, modes)
            period = rng.uniform(100.0, 400.0, modes)
            phase = rng.uniform(0.0, 2 * np.pi, modes)
            n = (w[:, None] * np.sin(2 * np.pi * t[None] / period[:, None] + phase[:, None])).sum(axis=0) / w.sum()      # [-1, 1]
            out[i, :, c] = (n + 1) * 0.5 * (hi - lo) + lo
    return out


def _simulate_moving_source(root, args, positions, name, src_y_pos, src_radius, num_frames, resolution, buoyancy, bWidth, open_bound,
                            time_step, adv_order, clamp_mode, scenes_per_batch, accuracy, device, preconditioner=None):
    """what the two generators below share: args.txt, the frames of every scene (scenes are batch entries), v_range.txt, n.npz"""
    from . import ops
    os.makedirs(os.path.join(root, "v"), exist_ok=True)
    with open(os.path.join(root, "args.txt"), "w") as f:
        for k, v in args:
            f.write("%s: %s\n" % (k, v))
    X, Y, Z = (int(n) for n in resolution)
    shape = (Z, Y, X)
    S, T = positions.shape[:2]
    sides = ops.open_sides(open_bound, 3)
    force = ops.default_buoyancy_force(shape, time_step, gravity=buoyancy)
    chunk = S if not scenes_per_batch else int(scenes_per_batch)
    v_range = [np.finfo(np.float64).max, np.finfo(np.float64).min]
    written = 0
    for c0 in range(0, S, chunk):
        part = list(range(c0, min(c0 + chunk, S)))
        pos = positions[part]                                                        # [b, T, 2]
        centers = np.stack([X * pos[..., 0], np.full(pos.shape[:2], Y * src_y_pos), Z * pos[..., 1]], axis=-1)      # gs * (px, y, pz)
        src = ops.SphereSource(torch.from_numpy(np.ascontiguousarray(centers.transpose(1, 0, 2), dtype=np.float32)).to(device), X * src_radius)
        d0 = torch.zeros((len(part),) + shape, dtype=torch.float32, device=device)
        v0 = torch.zeros((len(part),) + shape + (3,), dtype=torch.float32, device=device)
        frames = ops.simulate_smoke(d0, v0, T, dt=time_step, source=src, force=force, order=adv_order, clamp_mode=clamp_mode, bnd=bWidth,
                                    accuracy=accuracy, stack=False, open_bound=sides, preconditioner=preconditioner)
        for t, (_, v) in enumerate(frames):
            vh = v.cpu().numpy()
            v_range = [min(v_range[0], float(vh.min())), max(v_range[1], float(vh.max()))]
            for e, i in enumerate(part):
                y = np.full((2, num_frames), -1.0)                                   # the scripts' deque([-1]*num_frames, num_frames)
                y[:, num_frames - 1 - t:] = positions[i, :t + 1].T
                np.savez_compressed(os.path.join(root, "v", name(i, t)), x=vh[e], y=y)
                written += 1
    np.savez_compressed(os.path.join(root, "n.npz"), nx=positions[..., 0], nz=positions[..., 1])
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n" % v_range[0])
        f.write("%.3f" % v_range[1])
    return written


def generate_smoke3_rot_dataset(root, num_param=1, path_format="%d.npz", p0="frames", min_src_pos=0.1, max_src_pos=0.9, src_y_pos=0.1,
                                src_radius=0.08, circle_radius=0.25, circle_period=100, min_frames=0, max_frames=None, num_frames=500,
                                num_simulations=None, num_dof=2, resolution_x=48, resolution_y=72, resolution_z=48, buoyancy=-4e-3, bWidth=1,
                                open_bound="xXyYzZ", time_step=0.5, adv_order=2, clamp_mode=2, accuracy=1e-4, device="cuda",
                                preconditioner=None):
    """Simulate the reference's rotating-source set (scene/smoke3_rot.py, ``smoke3_rot_f500``) on the GPU and write it as that script
    does: ``args.txt`` with every argument of the script, ``v/%d.npz`` (x [Z,Y,X,3] float32 velocity after frame t, y [2, num_frames] =
    the last ``num_frames`` source positions (px; pz) as fractions of the grid, oldest first, padded in front with -1), ``n.npz`` (nx,
    nz [1, num_frames]) and ``v_range.txt``.  One scene: a sphere of radius ``X * src_radius`` at ``gs * (px, src_y_pos, pz)`` with
    ``px = 0.5 + circle_radius * cos(2 pi t / circle_period)``, ``pz`` the sine, all sides open by default.  The keyword arguments are
    the script's, with its defaults (``max_frames`` and ``num_simulations`` follow ``num_frames`` unless given).  The step is this
    library's restatement (include/deepfluids_hip.h: open sides, zero-gradient fill, plain CG; tests/smoke_open_ref.py), NOT
    mantaflow's.  Returns the number of files written."""
    if num_param != 1 or p0 != "frames":
        raise ValueError("generate_smoke3_rot_dataset: the scene has the one parameter frames")
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_frames if num_simulations is None else num_simulations
    args = [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("min_src_pos", min_src_pos),
            ("max_src_pos", max_src_pos), ("src_y_pos", src_y_pos), ("src_radius", src_radius), ("circle_radius", circle_radius),
            ("circle_period", circle_period), ("min_frames", min_frames), ("max_frames", max_frames), ("num_frames", num_frames),
            ("num_simulations", num_simulations), ("num_dof", num_dof), ("resolution_x", resolution_x), ("resolution_y", resolution_y),
            ("resolution_z", resolution_z), ("buoyancy", buoyancy), ("bWidth", bWidth), ("open_bound", open_bound), ("time_step", time_step),
            ("adv_order", adv_order), ("clamp_mode", clamp_mode)]
    t = np.arange(num_frames)
    positions = np.stack([0.5 + circle_radius * np.cos(t * 2 * np.pi / circle_period), 0.5 + circle_radius * np.sin(t * 2 * np.pi / circle_period)],
                         axis=-1)[None]
    return _simulate_moving_source(root, args, positions, lambda i, t: path_format % t, src_y_pos, src_radius, num_frames,
                                   (resolution_x, resolution_y, resolution_z), buoyancy, bWidth, open_bound, time_step, adv_order, clamp_mode,
                                   None, accuracy, device, preconditioner)


def generate_smoke3_mov_dataset(root, num_param=2, path_format="%d_%d.npz", p0="scenes", p1="frames", min_src_pos=0.1, max_src_pos=0.9,
                                src_y_pos=0.1, src_radius=0.08, min_scenes=0, max_scenes=None, num_scenes=200, min_frames=0, max_frames=None,
                                num_frames=400, num_simulations=None, num_dof=2, resolution_x=48, resolution_y=72, resolution_z=48,
                                buoyancy=-4e-3, bWidth=1, open_bound="xXyYzZ", time_step=0.5, adv_order=2, clamp_mode=2, nscale=0.01,
                                nrepeat=1000, nseed=123, positions=None, scenes_per_batch=None, accuracy=1e-4, device="cuda",
                                preconditioner=None):
    """Simulate the reference's moving-source set (scene/smoke3_mov.py, ``smoke3_mov200_f400``) on the GPU and write it as that script
    does: ``args.txt`` with every argument of the script, ``v/%d_%d.npz`` (scene, frame: x [Z,Y,X,3] float32 velocity after frame t, y
    [2, num_frames] = the last ``num_frames`` source positions (px; pz), oldest first, padded in front with -1), ``n.npz`` (nx, nz
    [num_scenes, num_frames]) and ``v_range.txt``.  Scenes are batch entries of ``ops.simulate_smoke`` (``scenes_per_batch`` splits
    them into chunks; an entry's result does not depend on the rest of its batch).  ``positions`` [num_scenes, num_frames, 2]: the
    source paths (px, pz) as fractions of the grid.  The default is ``smooth_source_paths(num_scenes, num_frames, min_src_pos,
    max_src_pos, seed=nseed)``, a seeded smooth path of this project's own: it is NOT the reference's Perlin noise, and ``nscale`` /
    ``nrepeat`` are written to args.txt but do not shape it.  The step is this library's restatement (include/deepfluids_hip.h: open
    sides, zero-gradient fill, plain CG; tests/smoke_open_ref.py), NOT mantaflow's.  Returns the number of files written."""
    if num_param != 2 or (p0, p1) != ("scenes", "frames"):
        raise ValueError("generate_smoke3_mov_dataset: the scene has the parameters (scenes, frames)")
    max_scenes = num_scenes - 1 if max_scenes is None else max_scenes
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_scenes * num_frames if num_simulations is None else num_simulations
    if positions is None:
        positions = smooth_source_paths(num_scenes, num_frames, min_src_pos, max_src_pos, seed=nseed)
    positions = np.asarray(positions, np.float64)
    if positions.shape != (num_scenes, num_frames, 2):
        raise ValueError("generate_smoke3_mov_dataset: positions must be [num_scenes, num_frames, 2] = %s, got %s" %
                         ((num_scenes, num_frames, 2), positions.shape))
    args = [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1), ("min_src_pos", min_src_pos),
            ("max_src_pos", max_src_pos), ("src_y_pos", src_y_pos), ("src_radius", src_radius), ("min_scenes", min_scenes),
            ("max_scenes", max_scenes), ("num_scenes", num_scenes), ("min_frames", min_frames), ("max_frames", max_frames),
            ("num_frames", num_frames), ("num_simulations", num_simulations), ("num_dof", num_dof), ("resolution_x", resolution_x),
            ("resolution_y", resolution_y), ("resolution_z", resolution_z), ("buoyancy", buoyancy), ("bWidth", bWidth),
            ("open_bound", open_bound), ("time_step", time_step), ("adv_order", adv_order), ("clamp_mode", clamp_mode), ("nscale", nscale),
            ("nrepeat", nrepeat), ("nseed", nseed)]
    return _simulate_moving_source(root, args, positions, lambda i, t: path_format % (i, t), src_y_pos, src_radius, num_frames,
                                   (resolution_x, resolution_y, resolution_z), buoyancy, bWidth, open_bound, time_step, adv_order, clamp_mode,
                                   scenes_per_batch, accuracy, device, preconditioner)


# ---- the noise-inflow scene (scene/smoke3_vel_buo.py): a cylinder source, a noise-modulated density inflow, an inflow velocity stamped
#      every frame, one inflow value and one buoyancy per scene ----
def smoke3_vel_buo_scenes(min_inflow, max_inflow, num_inflow, min_buoyancy, max_buoyancy, num_buoyancy):
    """``(p_list [S,2], pi_list [S,2])`` of scene/smoke3_vel_buo.py:144-153: the (inflow, buoyancy) values and their grid indices in the
    script's scene order, ``np.meshgrid(p1_space, p2_space).T.reshape(-1, 2)`` -- the buoyancy index runs fastest."""
    p_list = np.array(np.meshgrid(np.linspace(min_inflow, max_inflow, num_inflow), np.linspace(min_buoyancy, max_buoyancy, num_buoyancy))).T.reshape(-1, 2)
    pi_list = np.array(np.meshgrid(range(num_inflow), range(num_buoyancy))).T.reshape(-1, 2)
    return p_list, pi_list


def smoke3_vel_buo_inflow(resolution, src_x_pos=0.1, src_y_pos=0.25, src_z_pos=0.5, src_radius=0.14, src_height=0.04, time_step=0.5, nseed=123):
    """The ``ops.NoiseInflow`` of scene/smoke3_vel_buo.py for a grid ``resolution`` = (X, Y, Z): a cylinder at ``gs * (src_x_pos,
    src_y_pos, src_z_pos)`` of radius ``Y * src_radius`` and half-axis ``gs * (0, src_height, 0)``, the script's noise parameters with
    ``nseed`` seeding this project's own lattice noise (NOT mantaflow's wavelet noise), ``scale=1``, ``sigma=0.5``."""
    from . import ops
    X, Y, Z = (int(n) for n in resolution)
    shape = ops.CylinderShape((X * src_x_pos, Y * src_y_pos, Z * src_z_pos), (0.0, Y * src_height, 0.0), Y * src_radius)
    return ops.NoiseInflow(shape, ops.NoiseField(seed=nseed), scale=1.0, sigma=0.5, time_step=time_step)


def generate_smoke3_vel_buo_dataset(root, num_param=3, path_format="%d_%d_%d.npz", p0="inflow", p1="buoyancy", p2="frames", min_inflow=1,
                                    max_inflow=5, num_inflow=5, min_buoyancy=-2e-4, max_buoyancy=-10e-4, num_buoyancy=3, src_x_pos=0.1,
                                    src_y_pos=0.25, src_z_pos=0.5, src_radius=0.14, src_height=0.04, min_frames=0, max_frames=None,
                                    num_frames=250, num_simulations=None, resolution_x=112, resolution_y=64, resolution_z=32, bWidth=1,
                                    open_bound="XyY", time_step=0.5, adv_order=2, clamp_mode=2, scenes_per_batch=None, accuracy=1e-4,
                                    device="cuda", nseed=123, preconditioner=None):
    """Simulate the reference's inflow / buoyancy set (scene/smoke3_vel_buo.py:127-308, ``smoke3_vel5_buo3_f250``) on the GPU and write it
    as that script does: ``args.txt`` with every argument of the script in its order, ``v/%d_%d_%d.npz`` (x [Z,Y,X,3] float32 velocity
    after frame t, y = [inflow, buoyancy, t]) and ``v_range.txt``.  The keyword arguments are the script's, with its defaults
    (``max_frames`` and ``num_simulations`` follow ``num_frames`` and the grid of scenes unless given).  Per frame: the noise-modulated
    density inflow through the cylinder of ``smoke3_vel_buo_inflow``, the inflow velocity (p0, 0, 0) stamped into the cylinder's faces,
    both advections, resetOutflow, walls, buoyancy (0, p1, 0), projection, with the sides of ``open_bound`` open.  Scenes follow the
    script's meshgrid order and are batch entries of ONE ``ops.simulate_smoke`` with a per-entry inflow value and force
    (``scenes_per_batch`` splits them; an entry's result does not depend on the rest of its batch).  The step is this library's
    restatement (include/deepfluids_hip.h; tests/smoke_inflow_ref.py), NOT mantaflow's, and the noise is this project's OWN seeded
    lattice noise (``nseed``; it is not written to args.txt, which holds the script's keys only), not mantaflow's wavelet noise.
    Returns the number of files written."""
    from . import ops
    if num_param != 3 or (p0, p1, p2) != ("inflow", "buoyancy", "frames"):
        raise ValueError("generate_smoke3_vel_buo_dataset: the scene has the parameters (inflow, buoyancy, frames)")
    sides = ops.open_sides(open_bound, 3)
    max_frames = num_frames - 1 if max_frames is None else max_frames
    num_simulations = num_inflow * num_buoyancy * num_frames if num_simulations is None else num_simulations
    _write_args(root, [("log_dir", root), ("num_param", num_param), ("path_format", path_format), ("p0", p0), ("p1", p1), ("p2", p2),
                       ("min_inflow", min_inflow), ("max_inflow", max_inflow), ("num_inflow", num_inflow), ("min_buoyancy", min_buoyancy),
                       ("max_buoyancy", max_buoyancy), ("num_buoyancy", num_buoyancy), ("src_x_pos", src_x_pos), ("src_y_pos", src_y_pos),
                       ("src_z_pos", src_z_pos), ("src_radius", src_radius), ("src_height", src_height), ("min_frames", min_frames),
                       ("max_frames", max_frames), ("num_frames", num_frames), ("num_simulations", num_simulations),
                       ("resolution_x", resolution_x), ("resolution_y", resolution_y), ("resolution_z", resolution_z), ("bWidth", bWidth),
                       ("open_bound", open_bound), ("time_step", time_step), ("adv_order", adv_order), ("clamp_mode", clamp_mode)])
    X, Y, Z = int(resolution_x), int(resolution_y), int(resolution_z)
    shape = (Z, Y, X)
    p_list, pi_list = smoke3_vel_buo_scenes(min_inflow, max_inflow, num_inflow, min_buoyancy, max_buoyancy, num_buoyancy)
    inflow = smoke3_vel_buo_inflow((X, Y, Z), src_x_pos, src_y_pos, src_z_pos, src_radius, src_height, time_step, nseed)
    S = len(p_list)
    chunk = S if not scenes_per_batch else int(scenes_per_batch)
    v_range = [np.finfo(np.float64).max, np.finfo(np.float64).min]
    written = 0
    for c0 in range(0, S, chunk):
        part = list(range(c0, min(c0 + chunk, S)))
        values = torch.tensor([[p_list[i][0], 0.0, 0.0] for i in part], dtype=torch.float32, device=device)      # inflow = vec3(p0, 0, 0)
        force = ops.buoyancy_forces(shape, time_step, [p_list[i][1] for i in part]).to(device)                      # buoyancy = vec3(0, p1, 0)
        d0 = torch.zeros((len(part),) + shape, dtype=torch.float32, device=device)
        v0 = torch.zeros((len(part),) + shape + (3,), dtype=torch.float32, device=device)
        frames = ops.simulate_smoke(d0, v0, num_frames, dt=time_step, source=inflow, force=force, order=adv_order, clamp_mode=clamp_mode,
                                    bnd=bWidth, accuracy=accuracy, stack=False, open_bound=sides, inflow_velocity=(inflow.shape, values),
                                    preconditioner=preconditioner)
        for t, (_, v) in enumerate(frames):
            vh = v.cpu().numpy()
            v_range = [min(v_range[0], float(vh.min())), max(v_range[1], float(vh.max()))]
            for e, i in enumerate(part):
                np.savez_compressed(os.path.join(root, "v", path_format % (tuple(pi_list[i].tolist()) + (t,))), x=vh[e],
                                    y=[p_list[i][0], p_list[i][1], t])
                written += 1
    with open(os.path.join(root, "v_range.txt"), "w") as f:
        f.write("%.3f\n" % v_range[0])
        f.write("%.3f" % v_range[1])
    return written
