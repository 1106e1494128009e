"""CPU tests of ViTPose's single-product f16 mode: the ``precision=`` keyword, the library's new symbols and their argument checks, and
the restatement of the mode's arithmetic (tests/vitpose_f16_ref.py) against tests/vitpose_ref.py."""
import ctypes as C
import os.path as osp

import pytest
import torch

import vitpose_f16_ref as FR
import vitpose_ref as VR

TINY = dict(C=128, depth=1, heads=2, F1=32, F2=32, K=17)
TINY_IMG = (64, 48)
NEW_SYMBOLS = ("pmce_gemm_packed_f16_halves", "pmce_gemm_pack_f16", "pmce_gemm_nt_f16", "pmce_gemm_f16_set_tuning", "pmce_layernorm_rows_f16",
               "pmce_vit_attention_f16", "pmce_vitpose_create_precision", "pmce_vitpose_precision")


def test_an_unknown_precision_is_refused_before_any_device_work(monkeypatch):
    from pmce_amd import _lib, vitpose

    def no_library():
        raise AssertionError("the library was asked for before the precision was checked")

    monkeypatch.setattr(_lib, "load", no_library)
    sd = VR.state_dict(**TINY, img_size=TINY_IMG)
    for make in (lambda: vitpose.ViTPose({}, {}, "cuda:0", precision="bf16"),
                 lambda: vitpose.ViTPose.from_state_dict(sd, "cuda:0", img_size=TINY_IMG, precision="bf16"),
                 lambda: vitpose.ViTPose.from_checkpoint("/nonexistent/vitpose.pth", "cuda:0", precision="bf16")):
        with pytest.raises(ValueError) as err:
            make()
        assert '"split_f16"' in str(err.value) and '"f16"' in str(err.value) and "bf16" in str(err.value)
    with pytest.raises(ValueError, match="split_f16"):
        vitpose.vit_attention(torch.zeros(12, 384), 1, 12, 2, precision="fp8")
    with pytest.raises(ValueError, match='"f32", "planes" or "f16"'):
        vitpose.layernorm_rows(torch.zeros(4, 32), None, None, out="bf16")


def test_the_new_symbols_are_in_the_library_the_table_and_the_header():
    from pmce_amd import _lib, build
    build.build()
    lib = _lib.load()
    with open(osp.join(osp.dirname(osp.abspath(__file__)), "..", "include", "pmce_hip.h")) as fh:
        header = fh.read()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES and f" {name}(" in header, name


def test_the_entries_refuse_bad_arguments_and_name_the_value():
    from pmce_amd import _lib, build
    build.build()
    lib = _lib.load()
    P = 4096                                                    # a fake, aligned device pointer: the checks come before any launch

    def gemm(a=P, w=P, ws=P, bias=None, r=None, c=P, m=4, n=64, k=64, lda=None, ldc=None, act=0, c16=0):
        return lib.pmce_gemm_nt_f16(a, w, ws, bias, r, c, m, n, k, k if lda is None else lda, n if ldc is None else ldc, act, c16, None, None)

    for kw, word in ((dict(k=48), "K=48"), (dict(k=0), "K=0"), (dict(n=40), "N=40"), (dict(n=0), "N=0"), (dict(m=0), "M=0"), (dict(m=-3), "M=-3"),
                     (dict(a=None), "null pointer"), (dict(w=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(c=None), "null pointer"),
                     (dict(a=P + 8), "16-byte aligned"), (dict(c=P + 4), "16-byte aligned"), (dict(bias=P + 2), "16-byte aligned"),
                     (dict(act=2), "act must be 0 or 1 (got 2)"), (dict(lda=60), "lda=60"), (dict(ldc=32), "ldc=32"),
                     (dict(c16=1, r=P), "no residual")):
        assert gemm(**kw) == -1 and word in _lib.last_error(), (kw, _lib.last_error())
    assert lib.pmce_gemm_pack_f16(P, 64, 48, 48, P, P, None) == -1 and "K=48" in _lib.last_error()
    assert lib.pmce_gemm_pack_f16(P, 0, 64, 64, P, P, None) == -1 and "N=0" in _lib.last_error()
    assert lib.pmce_gemm_pack_f16(None, 64, 64, 64, P, P, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.pmce_gemm_packed_f16_halves(96, 64) == 128 * 64 and lib.pmce_gemm_packed_f16_halves(0, 64) == 0
    assert lib.pmce_layernorm_rows_f16(P, 4, 40, None, 0, None, P, P, 1e-6, P, None) == -1 and "C=40" in _lib.last_error()
    assert lib.pmce_layernorm_rows_f16(P, 4, 64, None, 0, None, P, P, 1e-6, None, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.pmce_layernorm_rows_f16(P, 4, 64, None, 0, None, P, P, 1e-6, P + 8, None) == -1 and "16-byte aligned" in _lib.last_error()
    assert lib.pmce_vit_attention_f16(P, P, 1, 200, 128, 2, None) == -1 and "N=200" in _lib.last_error()
    assert lib.pmce_vit_attention_f16(P, P, 1, 12, 96, 2, None) == -1 and "C=96" in _lib.last_error()
    assert lib.pmce_vit_attention_f16(P, None, 1, 12, 128, 2, None) == -1 and "null pointer" in _lib.last_error()
    assert lib.pmce_vit_attention_f16(P + 4, P, 1, 12, 128, 2, None) == -1 and "16-byte aligned" in _lib.last_error()
    h = C.c_void_p()
    for bad in (2, -1):
        assert lib.pmce_vitpose_create_precision(64, 48, 128, 1, 2, 32, 32, 17, bad, C.byref(h)) == -1
        assert f"got {bad}" in _lib.last_error() and "precision" in _lib.last_error()
    assert lib.pmce_vitpose_precision(None) == -1


def test_both_modes_list_the_same_tensors():
    from pmce_amd import _lib, build
    build.build()
    lib = _lib.load()
    tables = []
    for mode in (0, 1):
        h = C.c_void_p()
        assert lib.pmce_vitpose_create_precision(256, 192, 160, 2, 2, 32, 64, 17, mode, C.byref(h)) == 0
        assert lib.pmce_vitpose_precision(h) == mode
        shape = (C.c_int * 4)()
        rows = []
        for i in range(lib.pmce_vitpose_tensor_count(h)):
            rank = lib.pmce_vitpose_tensor_shape(h, i, shape)
            rows.append((lib.pmce_vitpose_tensor_name(h, i).decode(), rank, tuple(shape[:rank])))
        assert lib.pmce_vitpose_workspace_bytes(h, 3) > 0
        tables.append(rows)
        lib.pmce_vitpose_destroy(h)
    assert tables[0] == tables[1] and len(tables[0]) == 3 + 12 * 2 + 2 + 6
    h = C.c_void_p()
    assert lib.pmce_vitpose_create(64, 48, 128, 1, 2, 32, 32, 17, C.byref(h)) == 0 and lib.pmce_vitpose_precision(h) == 0
    lib.pmce_vitpose_destroy(h)


def test_the_restatement_without_rounding_is_the_reference():
    cfg = dict(H=TINY_IMG[0], W=TINY_IMG[1], **TINY)
    sd = VR.state_dict(**TINY, img_size=TINY_IMG)
    x = VR.patches(2, TINY_IMG)
    (h64, f64), _ = VR.run_both(sd, cfg, x)
    (hr, fr), _ = FR.run_both(sd, cfg, x, rnd=FR.identity)
    eh, ef = float((hr - h64).abs().max()), float((fr - f64).abs().max())
    print(f"identity rounding: heatmaps {eh:.2e}, features {ef:.2e}")
    assert eh <= 1e-12 and ef <= 1e-12
    (h16, f16), (dh, df) = FR.run_both(sd, cfg, x)
    assert float((h16 - h64).abs().max()) > 100 * eh and dh > 0 and df > 0          # and with r16 the mode really rounds


def test_r16_is_round_to_nearest_even_with_the_flush():
    g = torch.Generator().manual_seed(3)
    x = torch.cat([torch.randn(4096, generator=g) * 10.0 ** torch.randint(-6, 5, (4096,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 2.0 ** -14, -(2.0 ** -14), 2.0 ** -14 * (1 - 2.0 ** -12), 2.0 ** -15, 65504.0, 65519.0, 65520.0, -1e6,
                                 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, float("inf"), float("nan")])])
    want = torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(x), x).half().float()
    for dtype in (torch.float32, torch.float64):
        got = FR.r16(x.to(dtype)).float()
        assert torch.equal(torch.nan_to_num(got, nan=7.0), torch.nan_to_num(want, nan=7.0)), dtype
    assert float(FR.r16(torch.tensor(2.0 ** -14 * (1 - 2.0 ** -12)))) == 0.0               # below 2^-14: zero, not rounded up


def test_w16_of_a_wide_row_holds_no_subnormal():
    g = torch.Generator().manual_seed(11)
    k = 256
    w = (torch.rand(4, k, generator=g) * 2 - 1) * 2.0 ** (-20 * torch.rand(4, k, generator=g))        # a 2^-20 ... 1 spread inside each row
    w[:, 0] = torch.tensor([1.0, -0.75, 0.5, 0.9])
    w[2] *= 2.0 ** 12
    up = FR.row_scale(w)
    assert bool(((w.abs().amax(dim=1, keepdim=True) * up >= 2.0 ** 14) & (w.abs().amax(dim=1, keepdim=True) * up < 2.0 ** 15)).all())
    scaled = FR.w16(w) * up
    nz = scaled[scaled != 0].abs()
    assert float(nz.min()) >= 2.0 ** -14 and nz.numel() > 0.9 * w.numel()
    assert torch.equal(scaled, scaled.half().float())                                    # every entry is an f16 number
    assert torch.equal(FR.w16(w.double()).float(), FR.w16(w))                           # the same weight in the fp64 and the fp32 run


def test_gemm_f16_wrapper_refuses_mistyped_tensors():
    """The checks come before the library is touched: CPU tensors are enough."""
    from pmce_amd import vitpose
    pk = vitpose.PackedF16(torch.zeros(64 * 64, dtype=torch.float16), torch.ones(64), 64, 64)
    a = torch.zeros(4, 64, dtype=torch.float16)
    for kw, word in ((dict(a16=a.float()), "a16 must be"), (dict(a16=torch.zeros(64, 4, dtype=torch.float16).t()), "contiguous"),
                     (dict(out=torch.zeros(4, 64, dtype=torch.float16)), "out must be"), (dict(out=torch.zeros(4, 32)), "out must be"),
                     (dict(out_f16=True, out=torch.zeros(4, 64)), "out must be"), (dict(bias=torch.zeros(64, dtype=torch.float64)), "bias must be"),
                     (dict(bias=torch.zeros(32)), "bias must be"), (dict(residual=torch.zeros(4, 64, dtype=torch.float16)), "residual must be"),
                     (dict(residual=torch.zeros(4, 64), out_f16=True), "residual must be")):
        args = dict(a16=a, packed=pk)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            vitpose.gemm_f16(**args)
