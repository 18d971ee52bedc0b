"""GPU side of the density advection (advect.hip): the kernels against the fp64 restatement of tests/advect_ref.py with a tolerance
measured from its fp32 twin in the same test, bitwise cases, the sequence driver, the image kernel and ``Trainer.advect_``.

Each parity test prints, per case, e32 (fp32 twin vs fp64 over cells of equal branch), the kernel's largest error, the share of cells
left out and whether the kernel matched the twin bit for bit.  The twin's side of those figures (it needs no GPU; tests/test_advect_host.py
prints it): single steps e32 1.2e-07 .. 2.1e-06 with no cell left out, sequences of 8 steps e32 2.7e-06 (2-D) and 5.0e-07 (3-D) with at
most one interior cell of 35 532 taking another branch in a step."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import advect_ref as ref
from gpu_util import dev

pytestmark = pytest.mark.gpu


def _mask(src):
    return None if src is None else torch.from_numpy(src).cuda()


def _step_gpu(fx, kw, t=0, density=None):
    from deep_fluids_amd import ops
    d = dev(fx["density"]) if density is None else density
    return ops.advect(d, dev(fx["vels"][t]), fx["dt"], vel_scale=fx["vel_scale"], source=_mask(fx["source"]), **kw)


@pytest.mark.parametrize("shape", [(12, 9), (7, 8, 6), (128, 96), (19, 10, 7)])
def test_zero_velocity_bitwise(shape):
    from deep_fluids_amd import ops
    d = torch.rand((3,) + shape, generator=torch.Generator().manual_seed(1))
    v = torch.zeros((3,) + shape + (len(shape),))
    for bnd in (1, 2):
        want = np.where(ref.interior_mask(shape, bnd)[None], d.numpy(), 0).astype(np.float32)
        for order, mode in ((1, 2), (2, 1), (2, 2)):
            got = ops.advect(d.cuda(), v.cuda(), 0.5, order=order, clamp_mode=mode, bnd=bnd)
            np.testing.assert_array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(12, 10), (8, 9, 10), (128, 96)])
def test_exact_shift_bitwise(shape):
    from deep_fluids_amd import ops
    d, v, shift = ref.exact_shift_inputs(shape)
    for bnd in (1, 2):
        got = ops.advect(dev(d), dev(v), 0.5, order=1, bnd=bnd)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.shifted(d, shift, bnd))
        # the same displacement through vel_scale
        got = ops.advect(dev(d), dev(v / 4), 0.5, order=1, bnd=bnd, vel_scale=4.0)
        np.testing.assert_array_equal(got.cpu().numpy(), ref.shifted(d, shift, bnd))
        for mode in (1, 2):
            r64 = ref.step(d, v, 0.5, order=2, clamp_mode=mode, bnd=bnd, dtype=np.float64)
            got = ops.advect(dev(d), dev(v), 0.5, order=2, clamp_mode=mode, bnd=bnd)
            np.testing.assert_array_equal(got.cpu().numpy().astype(np.float64), r64["out"])


def test_single_step_parity_with_the_fp64_restatement():
    n = 0
    for name, fx, kw in ref.single_step_cases():
        args = dict(vel_scale=fx["vel_scale"], source=fx["source"], **kw)
        r64 = ref.step(fx["density"], fx["vels"][0], fx["dt"], dtype=np.float64, **args)
        r32 = ref.step(fx["density"], fx["vels"][0], fx["dt"], dtype=np.float32, **args)
        e32, twin_out = ref.twin_error(r64, r32, kw["bnd"])
        got = _step_gpu(fx, kw).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == fx["density"].shape
        raw = np.abs(got.astype(np.float64) - r64["out"])
        print("%-36s e32 %.3e  gpu max %.3e  twin left out %.5f %%  gpu == twin bitwise: %s" %
              (name, e32, float(raw.max()), 100 * twin_out, bool(np.array_equal(got, r32["out"]))))
        err, share = ref.compare(got, r64, e32, kw["bnd"],
                                 ref.alternatives_of(r64, fx["vels"][0], fx["dt"], kw["clamp_mode"], kw["bnd"], fx["vel_scale"]))
        print("%-36s gpu %.3e (bound %.3e)  left out %.5f %%" % ("", err, 3 * e32 + 1e-7, 100 * share))
        n += 1
    assert n == 36


def test_out_and_workspace_arguments():
    from deep_fluids_amd import ops
    name, fx, kw = next(c for c in ref.single_step_cases() if c[0] == "3d_16x24x16-o2-m2-b1-src")
    want = _step_gpu(fx, kw)
    d, v, m = dev(fx["density"]), dev(fx["vels"][0]), _mask(fx["source"])
    before = d.clone()
    ws = ops.advect_workspace(d, order=2, source=True)
    assert ws.numel() == 2 * d.numel()
    out = torch.empty_like(d)
    for _ in range(2):                                                   # the workspace is reusable
        got = ops.advect(d, v, fx["dt"], vel_scale=fx["vel_scale"], source=m, out=out, workspace=ws, **kw)
        assert got is out and torch.equal(out, want)
    assert torch.equal(d, before)                                        # the source is not stamped into the caller's density
    with pytest.raises(ValueError):
        ops.advect(d, v, fx["dt"], out=d)
    with pytest.raises(ValueError):
        ops.advect(d, v, fx["dt"], workspace=ws[:8])
    with pytest.raises(ValueError):
        ops.advect(d, v[..., :2].contiguous(), fx["dt"])
    # a mask of one grid is broadcast over the batch
    one = ops.advect(d, v, fx["dt"], vel_scale=fx["vel_scale"], source=m[0], **kw)
    assert torch.equal(one, want)


def test_sequence_equals_chained_steps_and_the_fp64_restatement():
    from deep_fluids_amd import ops
    for name, fx, kw in ref.sequence_cases():
        T = fx["vels"].shape[0]
        assert T == 8
        vels = dev(fx["vels"])
        d0 = dev(fx["density"])
        keep = d0.clone()
        final, imgs = ops.advect_sequence(d0, vels, fx["dt"], vel_scale=fx["vel_scale"], source=_mask(fx["source"]), images=True, **kw)
        assert torch.equal(d0, keep)
        d = d0
        frames = []
        for t in range(T):
            d = _step_gpu(fx, kw, t=t, density=d)
            frames.append(ops.density_image(d).cpu().numpy())
        assert torch.equal(final, d)                                                         # bitwise
        assert imgs.dtype == np.uint8 and imgs.shape == (T,) + fx["density"].shape[:1] + fx["density"].shape[-2:]
        np.testing.assert_array_equal(imgs, np.stack(frames))
        assert torch.equal(ops.advect_sequence(d0, list(vels), fx["dt"], vel_scale=fx["vel_scale"], source=_mask(fx["source"]), **kw), d)
        args = dict(vel_scale=fx["vel_scale"], source=fx["source"], **kw)
        s64 = ref.sequence(fx["density"], fx["vels"], fx["dt"], dtype=np.float64, **args)
        s32 = ref.sequence(fx["density"], fx["vels"], fx["dt"], dtype=np.float32, **args)
        e32, twin_out = ref.twin_error(s64[-1], s32[-1], kw["bnd"])
        got = final.cpu().numpy()
        print("%-36s e32 %.3e  gpu max %.3e  twin left out %.5f %%  gpu == twin bitwise: %s" %
              (name, e32, float(np.abs(got - s64[-1]["out"]).max()), 100 * twin_out, bool(np.array_equal(got, s32[-1]["out"]))))
        err, share = ref.compare(got, s64[-1], e32, kw["bnd"],
                                 ref.alternatives_of(s64[-1], fx["vels"][-1], fx["dt"], kw["clamp_mode"], kw["bnd"], fx["vel_scale"]))
        print("%-36s gpu %.3e (bound %.3e)  left out %.5f %%" % ("", err, 3 * e32 + 1e-7, 100 * share))


def test_density_image():
    from deep_fluids_amd import ops
    g = torch.Generator().manual_seed(4)
    for shape in ((3, 128, 96), (2, 9, 7), (1, 5, 8)):                   # 2-D: exact
        d = torch.rand(shape, generator=g) * 1.4 - 0.2                   # some values clip on either side
        got = ops.density_image(d.cuda())
        assert got.dtype == torch.uint8 and tuple(got.shape) == shape
        np.testing.assert_array_equal(got.cpu().numpy(), ref.density_image(d.numpy()))
    for shape in ((3, 16, 24, 16), (2, 19, 10, 7), (1, 64, 96, 64), (2, 5, 6, 12)):
        d = torch.rand(shape, generator=g) * 1.4 - 0.2
        got = ops.density_image(d.cuda()).cpu().numpy()
        want = ref.density_image(d.numpy())
        assert got.shape == want.shape == (shape[0], shape[2], shape[3])
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        n = int((diff != 0).sum())
        print("density image %-14s %7d pixels, %d differ, max step %d" % ("x".join(map(str, shape)), diff.size, n, int(diff.max())))
        assert diff.max() <= 1
        assert n <= 0.001 * diff.size, (shape, n)
        # against the float64 mean of the same data, the same rule
        w64 = np.clip((d.numpy().astype(np.float64).mean(axis=1)[:, ::-1]).astype(np.float32) * np.float32(255), 0, 255).astype(np.uint8)
        diff = np.abs(got.astype(np.int32) - w64.astype(np.int32))
        assert diff.max() <= 1 and int((diff != 0).sum()) <= 0.001 * diff.size


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _setup(tmp_path, is_3d, frames):
    from deep_fluids_amd import ops
    from deep_fluids_amd.data import BatchManager, write_synthetic_dataset
    from deep_fluids_amd.trainer import Trainer, Trainer3, default_config
    spatial = (8, 16, 8) if is_3d else (16, 8)
    root = str(tmp_path / "data")
    n = write_synthetic_dataset(root, spatial, num_p=(3, 2), num_frames=frames)
    cfg = default_config(is_3d=is_3d, res_x=8, res_y=16, res_z=8, filters=16, batch_size=2, num_samples=n, model_dir=str(tmp_path / "run"),
                         test_batch_size=2)
    dcfg = SimpleNamespace(random_seed=123, data_path=root, is_3d=is_3d, arch="de", data_type="velocity", batch_size=2,
                           res_x=8, res_y=16, res_z=8 if is_3d else 1, num_worker=1)
    ops.reset_variables()
    tr = (Trainer3 if is_3d else Trainer)(cfg)
    return tr, BatchManager(dcfg, device=None), spatial


def _test_dump_by_hand(tr, bm, p1, p2, y3, b):
    """What ``test_`` wrote before the sweep helper was factored out of it: the same statements, inline."""
    y1, y2 = int(bm.y_num[0]), int(bm.y_num[1])
    z_c = np.zeros((y3, tr.c_num), np.float32)
    z_c[:, 0] = p1 / float(y1 - 1) * 2 - 1
    z_c[:, 1] = p2 / float(y2 - 1) * 2 - 1
    z_c[:, -1] = np.linspace(-1, 1, num=y3)
    G = []
    for i in range(y3 // b):
        G_ = tr.generate(torch.from_numpy(z_c[b * i:b * (i + 1)]).to(tr.device)).cpu().numpy()
        G_, _ = bm.denorm(x=G_)
        G.append(G_)
    return z_c, np.concatenate(G, axis=0)


@pytest.mark.parametrize("is_3d", [False, True])
def test_trainer_advect(tmp_path, is_3d):
    from deep_fluids_amd import ops
    y3 = 6
    tr, bm, spatial = _setup(tmp_path, is_3d, y3)
    p1, p2 = 1, 1
    # test_'s dump is what the statements it consisted of produce
    z_c, G = _test_dump_by_hand(tr, bm, p1, p2, y3, 2)
    dump = tr.test_(bm, p1=p1, p2=p2)
    assert sorted(os.listdir(dump)) == sorted("%d.npz" % i for i in range(y3))
    for i in range(y3):
        with np.load(os.path.join(dump, "%d.npz" % i)) as f:
            np.testing.assert_array_equal(f["x"], G[i])
    source = {"center": (4.0, 3.0, 4.0)[:len(spatial)], "radius": 2.0}
    out_dir, final = tr.advect_(bm, p1=p1, p2=p2, source=source, dt=0.5)
    assert out_dir == os.path.join(dump, "d_adv")
    assert sorted(os.listdir(out_dir)) == ["%04d.png" % t for t in range(y3)]
    frames = torch.cat([tr.generate(torch.from_numpy(z_c[2 * i:2 * (i + 1)]).cuda()) for i in range(y3 // 2)], dim=0)
    mask = ops.sphere_mask(spatial, source["center"], source["radius"], "cuda")
    assert int(mask.sum()) > 0
    d0 = torch.zeros((1,) + spatial, device="cuda")
    want, imgs = ops.advect_sequence(d0, frames.unsqueeze(1), 0.5, vel_scale=float(bm.x_range), source=mask, images=True)
    assert final.is_cuda and torch.equal(final, want)                                        # bitwise
    assert float(final.max()) > 0
    for t in range(y3):
        png = _png(os.path.join(out_dir, "%04d.png" % t))
        assert png.dtype == np.uint8 and png.shape == spatial[-2:]                          # grey
        np.testing.assert_array_equal(png, imgs[t, 0])
    assert imgs.max() > 0
    # a mask in place of the sphere, the default time step (args.txt has no time_step: 0.5), order 1
    _, f1 = tr.advect_(bm, model_dir=str(tmp_path / "again"), p1=p1, p2=p2, source=mask.cpu().numpy(), order=1)
    w1 = ops.advect_sequence(d0, frames.unsqueeze(1), 0.5, order=1, vel_scale=float(bm.x_range), source=mask)
    assert torch.equal(f1, w1)
    assert len(os.listdir(str(tmp_path / "again" / ("%d_%d" % (p1, p2)) / "d_adv"))) == y3
    # test_ again after advect_: the same files
    dump2 = tr.test_(bm, p1=p1, p2=p2, model_dir=str(tmp_path / "dump2"))
    for i in range(y3):
        with np.load(os.path.join(dump2, "%d.npz" % i)) as f:
            np.testing.assert_array_equal(f["x"], G[i])
    ops.reset_variables()
