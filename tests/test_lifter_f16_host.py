"""The PMCE model's single-product f16 mode, the parts that need no GPU: the CPU restatement (tests/lifter_f16_ref.py) against the oracle,
its packing rule against the rule pmce_gemm_pack_f16 documents, and the mode's round trip on a handle."""
import ctypes as C
import os.path as osp
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, osp.dirname(osp.abspath(__file__)))

import lifter_f16_ref as LR  # noqa: E402


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_restatement_orders_its_yardsticks():
    """(J, C) = (17, 256), synthetic weights seed 123, inputs make_inputs(4, J, 321): the oracle's own fp32 noise is far below what f16
    operands cost, and the restatement's fp32 run sits between the two (an fp32-sized difference flips an f16 rounding)."""
    from pmce_amd import synth
    J, Cw = 17, 256
    sd = synth.make_state_dict(synth.lifter_spec(J, Cw, 3), seed=123)
    pose2d, img_feat = synth.make_inputs(4, J, 321)
    r = LR.run_both(sd, T(pose2d), T(img_feat), 3, "")
    print(f"J={J} C={Cw}: max |pose3d| {r['maxabs']:.0f} mm, dev32 {r['dev32']:.2e}, dev16 {r['dev16']:.2e}, dev32r {r['dev32r']:.2e} mm")
    assert r["dev32"] * 20 < r["dev32r"] < r["dev16"]
    assert r["dev16"] < 1.0          # the mode stays inside the 1e-3 m contract (pose3d is in mm)


def test_packing_rule_is_the_documented_one():
    """w16[n] = r16(w[n] 2^s) 2^-s with max |w[n]| 2^s in [2^14, 2^15), restated here in numpy's float16: rows with zeros, a zero row, products
    below 2^-14 (flushed, not sub-normal) and a maximum that is a power of two."""
    rng = np.random.default_rng(5)
    w = rng.standard_normal((8, 64)).astype(np.float32)
    w[0, ::3] = 0.0
    w[1] = 0.0
    w[2, :32] *= 1e-9                       # w 2^s far below 2^-14 beside a maximum near 1
    w[3, 5] = 2.0 ** -20                    # ... and exactly representable small values
    w[4] = np.clip(w[4], -0.5, 0.5)
    w[4, 7] = 0.5                           # the maximum is a power of two
    w[5] *= 1e-30
    w[6] *= 1e20
    w[7, 0] = -4.0
    w[7, 1:] = np.clip(w[7, 1:], -3.9, 3.9)
    m = np.abs(w).max(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        up = np.where(m > 0, 2.0 ** (14 - np.floor(np.log2(np.where(m > 0, m, 1.0)))), 1.0)
    scaled = w.astype(np.float64) * up
    assert ((np.abs(scaled).max(axis=1) >= 2 ** 14) | (m[:, 0] == 0)).all() and (np.abs(scaled).max(axis=1) < 2 ** 15).all()
    h = scaled.astype(np.float16).astype(np.float64)
    h[np.abs(scaled) < 2.0 ** -14] = 0.0
    want = h / up
    for dtype in (torch.float32, torch.float64):
        got = LR.w16(T(w).to(dtype))
        assert got.dtype == dtype and np.array_equal(got.double().numpy(), want)
    assert np.array_equal(LR.row_scale(T(w)).numpy(), up.astype(np.float32))
    assert (want[2, :32] == 0).all() and want[3, 5] == 2.0 ** -20 and want[4, 7] == 0.5 and want[7, 0] == -4.0


def test_mode_round_trips_on_a_handle():
    """pmce_model_set_gemm_mode(h, 2) / pmce_model_gemm_mode on a handle (creating one needs no GPU), value 3 refused, and the Python names."""
    from pmce_amd import _lib, models
    from pmce_amd.runtime import HipEngine
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.pmce_model_create(17, 512, 3, C.byref(h)) == 0
    assert lib.pmce_model_gemm_mode(h) == 1
    for mode in (2, 0, 2, 1):
        assert lib.pmce_model_set_gemm_mode(h, mode) == 0 and lib.pmce_model_gemm_mode(h) == mode
    for bad in (3, -1):
        assert lib.pmce_model_set_gemm_mode(h, bad) == -1 and "0 (fp32 pipe), 1 (split f16) or 2" in _lib.last_error()
        assert lib.pmce_model_set_gemm_mode_on(h, bad, None) == -1
    assert lib.pmce_model_gemm_mode(h) == 1
    lib.pmce_model_destroy(h)
    eng = HipEngine(17, 256, 3)
    assert eng.gemm_mode() == "split_f16"
    for mode in ("f16", "f32", "f16", "split_f16"):
        eng.set_gemm_mode(mode)
        assert eng.gemm_mode() == mode
    with pytest.raises(ValueError):
        eng.set_gemm_mode("f8")
    m = models.PMCE.get_model(17, 256, 3)
    m.set_gemm_mode("f16", min_batch=48)
    assert m._gemm_mode == "f16" and m._split_min_batch == 48
    m.set_gemm_mode(None)
    with pytest.raises(ValueError):
        m.set_gemm_mode("bf16")


def test_no_new_environment_variable(monkeypatch):
    """PMCE_SPLIT_F16 stays 0 or 1: the mode is opt-in through the API only."""
    from pmce_amd import _lib
    lib = _lib.load()
    monkeypatch.setenv("PMCE_SPLIT_F16", "2")
    h = C.c_void_p()
    assert lib.pmce_model_create(17, 256, 3, C.byref(h)) == 0
    assert lib.pmce_model_gemm_mode(h) == 1
    lib.pmce_model_destroy(h)


def test_form_arguments_are_checked_before_any_launch():
    """Form 3 of the row kernels and the attention entries, and form 0 / 3 of the new attention entry, are refused (no GPU is touched)."""
    from pmce_amd import _lib
    lib = _lib.load()
    p = 256
    assert lib.pmce_ln_chain_f32(p, 4, 256, None, None, 0.0, None, 1, 1, None, p, p, 1e-6, p, 3, None) == -1 and "out2_split" in _lib.last_error()
    assert lib.pmce_embed_ln_f32(p, p, p, p, p, p, 17, 17, 256, p, p, 1e-6, p, 3, None) == -1 and "xn_split" in _lib.last_error()
    assert lib.pmce_window_tokens_f32(p, p, p, p, p, 1e-6, p, p, 1, 16, 16, 17, 256, 3, None) == -1 and "xn_split" in _lib.last_error()
    assert lib.pmce_window_mid_tokens_f32(p, p, p, p, p, 1e-6, p, p, 1, 16, 16, 17, 256, 8, 3, None) == -1 and "xn_split" in _lib.last_error()
    assert lib.pmce_seq_attention_f32(p, p, 1, 17, 256, 0, 17, 0, 1, 3, None) == -1 and "out_split" in _lib.last_error()
    assert lib.pmce_lifter_attention_f32(p, p, 1, 17, 128, 0, 17, 0, 1, 3, None) == -1 and "out_split" in _lib.last_error()
    for form in (0, 3):
        assert lib.pmce_lifter_attention_split_f16_form(p, p, 1, 17, 128, 0, 17, 0, 1, form, None) == -1 and "out_form" in _lib.last_error()
    assert lib.pmce_lifter_attention_split_f16_form(p, p, 1, 18, 128, 0, 18, 0, 1, 2, None) == -1 and "16, 17 or 19" in _lib.last_error()
