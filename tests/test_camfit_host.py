"""CPU-only tests of the camera fit: the numpy restatement of the demo's loop (tests/camfit_ref.py) against the fixture made from the
real reference code (tests/golden/make_golden_camfit.py -> camfit.npz), the argument validation of the two C entry points, and the
Python-side chain tables."""
import ctypes as C

import numpy as np
import pytest

import camfit_ref as CR


@pytest.fixture(scope="module")
def fx(golden):
    return golden("camfit.npz")


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def test_fixture_statistics(fx):
    """What the fp32 GPU test is held to was measured on the reference's own fp32 run when the fixture was made."""
    assert int(fx["W"]) == CR.W and int(fx["seed"]) == CR.SEED and tuple(fx["snap_steps"]) == CR.SNAP_STEPS
    joints, target, _ = CR.windows()
    l64, l32 = CR.l1_loss(fx["cam64"], joints, target), CR.l1_loss(fx["cam32"], joints, target)
    share = float((np.abs(fx["cam32"].astype(np.float64) - fx["cam64"]).max(1) <= 1e-3).mean())
    assert share == float(fx["share32"]) >= 0.95
    assert float(((l32 - l64) / l64).max()) == pytest.approx(float(fx["excess32"]), rel=1e-9)
    assert 1e-4 < float(fx["excess32"]) < 1e-2


def test_numpy_restatement_matches_reference_fp64(fx):
    """The loop without autograd reproduces the reference's fp64 run on all 200 windows and at every stored step count to 1e-12
    (measured: 7.5e-16 at 300 steps, 1.1e-16 after steps 1 and 2)."""
    joints, target, init = CR.windows()
    cam, snaps = CR.fit(joints, target, init, snapshots=CR.SNAP_STEPS)
    for k, s in enumerate(CR.SNAP_STEPS):
        d = float(np.abs(snaps[k] - fx["snaps64"][k]).max())
        print(f"steps {s}: max |restatement - reference fp64| = {d:.2e}")
        assert d <= 1e-12, (s, d)
    assert np.array_equal(snaps[-1], cam)
    assert float(np.abs(cam - fx["cam64"]).max()) <= 1e-12
    assert np.array_equal(fx["snaps64"][-1], fx["cam64"])


def test_numpy_restatement_chain(fx):
    """The demo's carry along a tracklet.  Every link - window k restarted from the FIXTURE's camera k - 1 - reproduces the fixture's
    camera k to 1e-12 (measured 1.1e-16).  The free-running chain of 40 sits 3.4e-12 from the fixture: the reference run's square
    roots are its math library's (1 ulp off the IEEE result for 1.2 % of arguments, measured on the machine that made the fixture),
    which numpy does not reproduce, and a chain hands each window's last-bit difference to the next, where some windows amplify it.
    So the free run is held to the 1e-9 the GPU tests use for "same algorithm, different rounding", the links to 1e-12."""
    joints, target, init = CR.windows()
    n = CR.CHAIN_LEN
    ref = fx["chain64"]
    start = np.concatenate([init[:1].astype(np.float64), ref[:-1]])
    links = CR.fit(joints[:n], target[:n], start)
    d_link = float(np.abs(links - ref).max())
    free = CR.fit_chain(joints[:n], target[:n], init[0])
    d_free = float(np.abs(free - ref).max())
    print(f"chain of {n}: links {d_link:.2e}, free-running {d_free:.2e}")
    assert d_link <= 1e-12
    assert d_free <= 1e-9
    assert float(np.abs(ref[1] - fx["cam64"][1]).max()) > 1e-6          # a carried start is not the window's own init


def test_orig_cam_restatement(fx):
    got = CR.orig_cam(fx["cam64"][:len(fx["boxes"])], fx["boxes"], *fx["img_wh"])
    assert np.allclose(got, fx["orig_cam"], rtol=1e-12, atol=0)
    b = fx["boxes"].astype(np.float64)
    off = np.abs(b[:, 0] + b[:, 2] / 2 - fx["img_wh"][0] / 2)
    assert off[0] == 0 and (off[1:] > 10).all()                           # one centred box, the rest are not


def test_step_table():
    from pmce_amd import camera
    tab = camera.step_table()
    assert tab.shape == (300, 2) and tab.dtype == np.float64
    for t, lr in ((1, 0.1), (101, 0.1), (102, 0.05), (201, 0.05), (202, 0.001), (300, 0.001)):
        assert tab[t - 1, 0] == lr / (1 - 0.9 ** t) and tab[t - 1, 1] == (1 - 0.999 ** t) ** 0.5, t
    short = camera.step_table(5, lrs=(1.0, 0.5, 0.25), lr_switch=(0, 2))
    assert [round(short[j, 0] * (1 - 0.9 ** (j + 1)), 12) for j in range(5)] == [1.0, 0.5, 0.5, 0.25, 0.25]
    with pytest.raises(ValueError):
        camera.step_table(0)


def test_chain_tables():
    from pmce_amd import camera
    assert camera.resolve_chains(7) is None
    one = camera.resolve_chains(7, chain=True)
    assert one.dtype == np.int32 and one.tolist() == [0, 7]                   # chain=True: the single chain over all windows
    assert camera.resolve_chains(7, [0, 3, 3, 7], chain=True).tolist() == [0, 3, 3, 7]
    for bad, msg in (([1, 7], "start at 0"), ([0, 6], "end at W"), ([0, 5, 4, 7], "monotone"), ([0], ">= 2 entries"), ([0.0, 7.0], "integer"),
                     ([[0, 7]], "1-D")):
        with pytest.raises(ValueError, match=msg):
            camera.check_seq_offsets(bad, 7)
    init = camera.default_init(3, seed=5)
    assert tuple(init.shape) == (3, 3) and float(init.min()) >= 0 and float(init.max()) < 1
    assert np.array_equal(init.numpy(), camera.default_init(3, seed=5).numpy())


def _call(lib, name, W=4, S=4, n_fit=17, n_target=19, steps=300, seq=None, seq_dev=None, bbox=None, orig=None, img=(0.0, 0.0), crop=500.0):
    seq_host = None if seq is None else (C.c_int * len(seq))(*seq)
    return getattr(lib, name)(16, 16, 16, seq_host, seq_dev, 16, 16, 16, bbox, orig, W, S, n_fit, n_target, steps, 1.0, crop, img[0], img[1], None)


@pytest.mark.parametrize("name", ["pmce_camfit_f32", "pmce_camfit_f64"])
def test_camfit_argument_validation_without_gpu(lib, name):
    """Every bad argument is refused on the host, before any launch, with its own message."""
    from pmce_amd import _lib
    for kw, msg in ((dict(n_fit=0), "n_fit must be in 1..32"), (dict(n_fit=33, n_target=40), "n_fit must be in 1..32"),
                    (dict(steps=0), "steps must be >= 1"),
                    (dict(n_target=16), "fewer than n_fit"),
                    (dict(S=2, seq=[0, 2, 4], seq_dev=None), "on the host and on the device"),
                    (dict(S=2, seq=[1, 2, 4], seq_dev=16), "start at 0 and end at W"),
                    (dict(S=2, seq=[0, 2, 5], seq_dev=16), "start at 0 and end at W"),
                    (dict(S=3, seq=[0, 3, 2, 4], seq_dev=16), "monotone"),
                    (dict(S=2), "S must equal W"),
                    (dict(bbox=16), "go together"), (dict(bbox=16, orig=16), "go together"), (dict(img=(1920.0, 1080.0)), "go together"),
                    (dict(bbox=16, orig=16, img=(1920.0, 0.0)), "go together"),
                    (dict(crop=0.0), "crop_size must be positive"), (dict(W=0, S=0), "W and S must be >= 1")):
        assert _call(lib, name, **kw) == -1, kw
        assert msg in _lib.last_error() and name[5:] in _lib.last_error(), (kw, _lib.last_error())


def test_fit_camera_checks_its_arguments():
    import torch
    from pmce_amd import camera
    j, t = torch.zeros(4, 17, 3), torch.zeros(4, 19, 2)
    for args, kw, msg in (((torch.zeros(4, 33, 3), torch.zeros(4, 40, 2)), {}, "1..32"), ((j, torch.zeros(4, 16, 2)), {}, "target2d"),
                          ((j, torch.zeros(3, 19, 2)), {}, "target2d"), ((j, t), dict(precision="f16"), "precision"),
                          ((j, t), dict(bbox=torch.zeros(4, 4)), "go together"), ((j, t), dict(seq_offsets=[0, 3]), "end at W"),
                          ((j, t), dict(steps=0), "steps"), ((torch.zeros(4, 17, 2), t), {}, "joints3d")):
        with pytest.raises(ValueError, match=msg):
            camera.fit_camera(*args, **kw)
