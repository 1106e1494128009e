"""The PMCE model's opt-in single-product f16 mode, ``set_gemm_mode("f16")``, through the drop-in modules on the GPU.

The reference is tests/lifter_f16_ref.py: the mode restated on the CPU over the oracle (r16 operands, w16 weights in the lifter blocks'
products; everything else the oracle's).  Bounds, in the project's FACTOR = 4 (tests/vitpose_f16_ref.py): the device within
FACTOR x dev32r of the restatement's fp64 run and within FACTOR x dev16 of the oracle's fp64 run, every measured ratio printed; the
absolute deviation inside the path's 1e-3 m contract.  The weights are synthetic: nothing here is an accuracy claim on a real checkpoint."""
import os.path as osp
import sys

import numpy as np
import pytest
import torch

from conftest import cached_state_dict

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

import lifter_f16_ref as LR  # noqa: E402

pytestmark = pytest.mark.gpu

FACTOR, TOL_M = LR.FACTOR, LR.TOL_M
_LIFTERS, _MODELS = {}, {}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def lifter_sd(J, C):
    from pmce_amd import synth
    return synth.make_state_dict(synth.lifter_spec(J, C, 3), seed=123)


def new_lifter(J, C, sd):
    from pmce_amd import models
    m = models.PoseEstimation.get_model(J, C, 3)
    m.load_state_dict(sd)
    return m.to(dev())


def get_lifter(J, C):
    """(module, its lifter-only state_dict) - no 412 MB model around the lifter; one resident at a time."""
    if (J, C) not in _LIFTERS:
        _LIFTERS.clear()
        sd = lifter_sd(J, C)
        _LIFTERS[(J, C)] = (new_lifter(J, C, sd), sd)
    return _LIFTERS[(J, C)]


def get_model(J=17, C=256):
    from pmce_amd import assets, models
    if (J, C) not in _MODELS:
        _MODELS.clear()
        torch.cuda.empty_cache()
        m = models.PMCE.get_model(J, C, 3)
        m.load_state_dict(cached_state_dict(J, C))
        m.set_j_regressor(assets.load_j_regressor("h36m"))
        _MODELS[(J, C)] = m.to(dev())
    return _MODELS[(J, C)]


def run_mode(m, mode, *inputs, call=None, min_batch=1):
    """The module's result in `mode` (the module is left in the library's default mode)."""
    m.set_gemm_mode(mode, min_batch=min_batch)
    try:
        if mode is not None:
            assert m.gemm_mode() == mode
        out = (call or m)(*inputs)
        torch.cuda.synchronize()
        return out.clone() if torch.is_tensor(out) else tuple(o.clone() for o in out)
    finally:
        m.set_gemm_mode(None)


def held(what, got, ref64, plain64, dev32r, dev16, scale_to_m):
    """Print the measured ratios, then the two FACTOR bounds and the contract."""
    e_ref, e_plain = maxabs(got, ref64), maxabs(got, plain64)
    print(f"{what}: vs restatement {e_ref:.3e} = {e_ref / dev32r:.2f} x dev32r ({dev32r:.3e}); vs oracle fp64 {e_plain:.3e} = "
          f"{e_plain / dev16:.2f} x dev16 ({dev16:.3e})")
    assert e_ref <= FACTOR * dev32r, f"{what}: {e_ref / dev32r:.2f} x dev32r"
    assert e_plain <= FACTOR * dev16, f"{what}: {e_plain / dev16:.2f} x dev16"
    assert e_plain * scale_to_m < TOL_M
    return e_ref / dev32r, e_plain / dev16


@pytest.mark.parametrize("J,C", [(17, 128), (17, 256), (19, 384), (17, 512)])
def test_lifter_against_the_restatement(J, C):
    from pmce_amd import synth
    B = 3
    m, sd = get_lifter(J, C)
    pose2d, img_feat = synth.make_inputs(B, J, 321)
    r = LR.run_both(sd, T(pose2d), T(img_feat), 3, "")
    p, f = T(pose2d).to(dev()), T(img_feat).to(dev())
    out = run_mode(m, "f16", p, f)
    split = run_mode(m, "split_f16", p, f)
    print(f"J={J} C={C} B={B}: max |pose3d| {r['maxabs']:.0f} mm, dev32 {r['dev32']:.2e}, dev16 {r['dev16']:.2e}, dev32r {r['dev32r']:.2e} mm; "
          f"split mode vs oracle fp64 {maxabs(split, r['plain64']):.2e} mm")
    held(f"pose3d J={J} C={C} (mm)", out, r["ref64"], r["plain64"], r["dev32r"], r["dev16"], 1e-3)
    assert maxabs(out, split) > 1e-3, "the mode is really in use: its result is not the split mode's"


def test_a_clip_does_not_depend_on_its_batch_at_512():
    """C = 512: clip 0 has the same bits at B = 1 (M = 272, below one tile), 3 and 33 (561 temporal sequences: the persistent attention grid
    wraps; and the threshold of the fused qkv + attention kernel, which this mode must not take).  Clips 0, 16, 32 of B = 33 against the
    restatement run on those three clips alone."""
    from pmce_amd import synth
    J, C = 17, 512
    m, sd = get_lifter(J, C)
    pose2d, img_feat = synth.make_inputs(33, J, 11)
    p, f = T(pose2d).to(dev()), T(img_feat).to(dev())
    m.set_gemm_mode("f16", min_batch=1)
    try:
        outs = {b: m(p[:b], f[:b]).clone() for b in (1, 3, 33)}
        torch.cuda.synchronize()
    finally:
        m.set_gemm_mode(None)
    assert torch.equal(outs[1][0], outs[3][0]) and torch.equal(outs[1][0], outs[33][0])
    assert torch.equal(outs[3], outs[33][:3])
    pick = [0, 16, 32]
    r = LR.run_both(sd, T(pose2d[pick]), T(img_feat[pick]), 3, "")
    held("pose3d clips 0, 16, 32 of B=33, C=512 (mm)", outs[33][pick], r["ref64"], r["plain64"], r["dev32r"], r["dev16"], 1e-3)


def test_full_model_against_the_restatement():
    from pmce_amd import synth
    J, C, B = 17, 256, 2
    model = get_model(J, C)
    sd = cached_state_dict(J, C)
    pose2d, img_feat = synth.make_inputs(B, J, 321)
    ref64, plain64, dev32r, dev16 = LR.run_both_model(sd, T(pose2d), T(img_feat), model.vj_relation)
    out = run_mode(model, "f16", T(pose2d).to(dev()), T(img_feat).to(dev()))
    for k, (name, to_m) in enumerate((("mesh (m)", 1.0), ("pose (m)", 1.0), ("pose3d (mm)", 1e-3))):
        held(f"PMCE J={J} C={C} B={B} {name}", out[k], ref64[k], plain64[k], dev32r[k], dev16[k], to_m)


def test_default_modes_keep_their_bits():
    """'split_f16' and 'f32' results taken before any 'f16' call equal those taken after switching back, and those of a fresh module."""
    from pmce_amd import synth
    J, C = 17, 256
    sd = lifter_sd(J, C)
    m = new_lifter(J, C, sd)
    p, f = (T(a).to(dev()) for a in synth.make_inputs(3, J, 9))
    before = {mode: run_mode(m, mode, p, f) for mode in ("split_f16", "f32", None)}
    mid = run_mode(m, "f16", p, f)
    after = {mode: run_mode(m, mode, p, f) for mode in ("split_f16", "f32", None)}
    fresh = new_lifter(J, C, sd)
    for mode in before:
        assert torch.equal(before[mode], after[mode]), mode
        assert torch.equal(before[mode], run_mode(fresh, mode, p, f)), mode
    assert torch.equal(before[None], before["split_f16"]) and not torch.equal(mid, before["split_f16"])
    assert torch.equal(mid, run_mode(fresh, "f16", p, f))


def test_min_batch_keeps_small_calls_on_the_fp32_pipe():
    from pmce_amd import synth
    J, C = 17, 256
    m, _ = get_lifter(J, C)
    p, f = (T(a).to(dev()) for a in synth.make_inputs(4, J, 10))
    assert torch.equal(run_mode(m, "f16", p, f, min_batch=48), run_mode(m, "f32", p, f))
    assert not torch.equal(run_mode(m, "f16", p, f, min_batch=4), run_mode(m, "f32", p, f))


def test_overflow_is_reported_or_rerun_on_the_fp32_pipe():
    """One mlp.fc1.bias element at 7e4 pushes a GELU result past f16's 65504: 'report' shows it, the default 'rerun' computes the batch again
    on the fp32 pipe - the bits of 'f32' mode - and a later call on clean weights is unaffected."""
    from pmce_amd import synth
    J, C, B = 17, 256, 2
    sd = lifter_sd(J, C)
    bad = {k: v.clone() for k, v in sd.items()}
    bad["SpatialBlocks.1.mlp.fc1.bias"][5] = 7.0e4
    p, f = (T(a).to(dev()) for a in synth.make_inputs(B, J, 77))
    m = new_lifter(J, C, sd)
    m.set_gemm_mode("f16", min_batch=1)
    clean = m(p, f).clone()
    assert m.overflow_reruns == 0 and not m.overflowed() and bool(torch.isfinite(clean).all())
    m.load_state_dict(bad)
    m.set_overflow_policy("report")
    out = m(p, f)
    assert m.overflowed() and not bool(torch.isfinite(out).all())
    m.clear_overflow()
    m.set_overflow_policy("rerun")
    out = m(p, f).clone()
    assert m.overflow_reruns == 1 and not m.overflowed() and bool(torch.isfinite(out).all())
    m.set_gemm_mode("f32")
    assert torch.equal(out, m(p, f)), "a re-run is the fp32 pipe's result, bit for bit"
    m.load_state_dict(sd)
    m.set_gemm_mode("f16", min_batch=1)
    assert torch.equal(m(p, f), clean) and m.overflow_reruns == 1 and not m.overflowed()


def test_graph_pipeline_and_streaming_inherit_the_mode():
    from pmce_amd import streaming, synth
    J, C = 17, 256
    model = get_model(J, C)
    sd = cached_state_dict(J, C)
    model.set_gemm_mode("f16", min_batch=1)
    try:
        assert model.gemm_mode() == "f16"
        # a captured graph
        p1, f1 = (T(a).to(dev()) for a in synth.make_inputs(1, J, 5))
        eager = [t.clone() for t in model.forward_with_joints(p1, f1)]
        got = model.graphed(1)(p1, f1)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, got))
        # two pipeline lanes on the shared arena
        batches = [tuple(T(a).to(dev()) for a in synth.make_inputs(b, J, 700 + i)) for i, b in enumerate((5, 3, 5, 1))]
        direct = [tuple(t.clone() for t in model.forward_with_joints(p, f)) for p, f in batches]
        pipe = model.pipeline(depth=2)
        tickets = [pipe.submit(p, f) for p, f in batches]
        for d, t in zip(direct, tickets):
            assert all(torch.equal(a, b) for a, b in zip(d, t.result()))
        assert not pipe.synchronize()
        # a streamed sequence
        L = 20
        p_np, f_np = synth.make_inputs(2, J, 5)
        pose_fr, feat_fr = T(p_np.reshape(-1, J, 2)[:L]).to(dev()), T(f_np.reshape(-1, 2048)[:L]).to(dev())
        win = streaming.demo_window_list(L)
        wp, wf = streaming.assemble_windows(pose_fr, feat_fr, win)
        out = streaming.stream_forward(model, pose_fr, feat_fr, windows=win, batch=16)
        direct = model(wp, wf)
        torch.cuda.synchronize()
    finally:
        model.set_gemm_mode(None)
    split = streaming.stream_forward(model, pose_fr, feat_fr, windows=win, batch=16)
    r = LR.run_both(sd, wp.cpu(), wf.cpu(), 3, "pose_lifter.")
    held(f"streamed pose3d, L={L} (mm)", out[2], r["ref64"], r["plain64"], r["dev32r"], r["dev16"], 1e-3)
    assert maxabs(out[0], direct[0]) < TOL_M and maxabs(out[2], split[2]) > 1e-3
