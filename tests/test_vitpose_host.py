"""CPU tests of the host side of the ViTPose network (pmce_amd/vitpose.py, synth.vitpose_spec, tests/vitpose_ref.py): the state-dict
selection, the variant inference, the deconvolution as a product and a gather, the synthetic spec's attention, the library's symbols."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vitpose_ref as VR
from pmce_amd import synth

TINY = dict(C=128, depth=1, heads=2, F1=32, F2=32, K=17)
TINY_IMG = (64, 48)


@pytest.fixture(scope="module")
def sd():
    return VR.state_dict(**TINY, img_size=TINY_IMG)


def test_selection_accepts_prefixes_and_ignores_foreign_heads(sd):
    from pmce_amd import vitpose
    full = {"module." + k: v for k, v in sd.items()}
    full.update({"module.associate_keypoint_heads.0.final_layer.weight": torch.zeros(14, 32, 1, 1), "epoch": torch.tensor(3),
                 "module.keypoint_head.deconv_layers.1.num_batches_tracked": torch.tensor(7)})
    cfg, t = vitpose.select_state_dict(full, img_size=TINY_IMG)
    cfg0, t0 = vitpose.select_state_dict(sd, img_size=TINY_IMG)
    assert cfg == cfg0 == dict(H=64, W=48, **TINY)
    assert list(t) == list(t0) == list(vitpose.required_keys(cfg)) and all(torch.equal(t[k], t0[k]) for k in t)
    assert not any("associate" in k or "num_batches" in k for k in t)
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in t.values())


def test_selection_errors_name_the_tensor(sd):
    from pmce_amd import vitpose
    for name in ("backbone.blocks.0.mlp.fc2.bias", "keypoint_head.deconv_layers.4.running_var", "backbone.last_norm.weight"):
        broken = {k: v for k, v in sd.items() if k != name}
        with pytest.raises(ValueError, match=name.replace(".", r"\.")):
            vitpose.select_state_dict(broken, img_size=TINY_IMG)
    broken = dict(sd)
    broken["backbone.blocks.0.attn.qkv.weight"] = torch.zeros(3 * 128, 64)
    with pytest.raises(ValueError, match=r"backbone\.blocks\.0\.attn\.qkv\.weight.*\(384, 64\)"):
        vitpose.select_state_dict(broken, img_size=TINY_IMG)
    with pytest.raises(ValueError, match="backbone.pos_embed"):
        vitpose.select_state_dict({"epoch": 1})
    with pytest.raises(ValueError, match="img_size"):
        vitpose.select_state_dict(sd)                           # 256 x 192 is 192 tokens, the tensors have 12
    with pytest.raises(ValueError, match="mapping"):
        vitpose.select_state_dict([1, 2])
    with pytest.raises(ValueError, match="num_heads=3"):
        vitpose.select_state_dict(sd, img_size=TINY_IMG, num_heads=3)


@pytest.mark.parametrize("name,C,depth,heads", [("B", 768, 12, 12), ("L", 1024, 24, 16), ("H", 1280, 32, 16)])
def test_variant_inference(name, C, depth, heads):
    """The published B, L and H shapes, on stand-ins that carry a shape and no storage."""
    from pmce_amd import vitpose
    spec = synth.vitpose_spec(C, depth, heads, 256, 256, 17)
    meta = {k: torch.empty(shape, device="meta") for k, (shape, _, _) in spec.items()}
    meta["associate_keypoint_heads.0.final_layer.weight"] = torch.empty(14, 256, 1, 1, device="meta")
    cfg = vitpose.infer_config(meta)
    assert cfg == dict(H=256, W=192, C=C, depth=depth, heads=heads, F1=256, F2=256, K=17), name
    assert vitpose.infer_config(meta, num_heads=C // 64)["heads"] == C // 64
    assert list(vitpose.required_keys(cfg)) == [k for k in spec]


@pytest.mark.parametrize("h,w", [(4, 3), (16, 12)])
def test_deconvolution_is_a_product_and_a_gather(h, w):
    from pmce_amd import vitpose
    g = torch.Generator().manual_seed(h)
    n, cin, cout = 2, 24, 16
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64) / 8
    gamma, beta, mean = (torch.randn(cout, generator=g, dtype=torch.float64) for _ in range(3))
    var = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5
    want = F.relu(F.batch_norm(F.conv_transpose2d(x, wt, stride=2, padding=1), mean, var, gamma, beta, False, 0.0, 1e-5))
    wf, bf = vitpose.fold_bn_deconv(wt, gamma, beta, mean, var)
    assert wf.dtype == torch.float64 and bf.dtype == torch.float32
    bf64 = beta - mean * gamma / torch.sqrt(var + 1e-5)
    wp = vitpose.deconv_weight_as_product(wf)
    assert wp.shape == (16 * cout, cin)
    y = x.permute(0, 2, 3, 1).reshape(n * h * w, cin) @ wp.T
    got = vitpose.deconv_gather_host(y, bf64, n, h, w).permute(0, 3, 1, 2)
    assert got.shape == want.shape == (n, cout, 2 * h, 2 * w)
    err = float((got - want).abs().max())
    print(f"deconvolution {h} x {w}: max error {err:.2e}")
    assert err <= 1e-12
    assert float((bf.double() - bf64).abs().max()) < 1e-6
    with pytest.raises(ValueError, match="4 x 4"):
        vitpose.deconv_weight_as_product(torch.zeros(3, 2, 3, 3))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 3), (3, 1)])
def test_gather_definition_at_a_one_pixel_side(h, w):
    """H = 1 or W = 1: every output pixel is a border pixel and ky = 0 / 3 (kx = 0 / 3) reaches no output row (column) at all."""
    from pmce_amd import vitpose
    g = torch.Generator().manual_seed(10 * h + w)
    n, cin, cout = 2, 24, 16
    x = torch.randn(n, cin, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn(cin, cout, 4, 4, generator=g, dtype=torch.float64) / 8
    bias = torch.randn(cout, generator=g, dtype=torch.float64) * 0.3
    want = F.relu(F.conv_transpose2d(x, wt, bias, stride=2, padding=1))
    y = x.permute(0, 2, 3, 1).reshape(n * h * w, cin) @ vitpose.deconv_weight_as_product(wt).T
    got = vitpose.deconv_gather_host(y, bias, n, h, w).permute(0, 3, 1, 2)
    assert got.shape == want.shape == (n, cout, 2 * h, 2 * w)
    err = float((got - want).abs().max())
    print(f"deconvolution {h} x {w}: max error {err:.2e}")
    assert err <= 1e-12
    assert 0.2 < float((want > 0).double().mean()) < 0.8


def test_synthetic_attention_is_neither_uniform_nor_one_hot():
    """The reference's attention rows at the demo's 192 tokens, on the synthetic spec: the median of their largest probability lies
    between 0.02 (well above the uniform 1 / 192) and 0.9 (below one-hot)."""
    cfg = dict(C=160, depth=2, heads=2, F1=32, F2=32, K=17)
    sd = VR.state_dict(**cfg)
    m = VR.module(sd, **cfg, dtype=torch.float64)
    with torch.no_grad():
        m(VR.patches(1).double())
    for i, b in enumerate(m.backbone.blocks):
        p = b.attn.last_probs
        assert p.shape == (1, 2, 192, 192)
        med = float(p.max(dim=-1).values.median())
        print(f"block {i}: median largest probability {med:.3f}")
        assert 0.02 < med < 0.9
    w = sd["backbone.blocks.0.attn.qkv.weight"]
    assert float(w[:320].abs().max()) > 1.5 * float(w[320:].abs().max())    # the q and k rows are the wide ones


def test_the_spec_is_the_reference_modules_layout():
    cfg = dict(C=128, depth=2, heads=2, F1=32, F2=64, K=5)
    spec = synth.vitpose_spec(**cfg, img_size=TINY_IMG)
    m = VR.ViTPoseRef(**cfg, img_size=TINY_IMG)
    want = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.endswith("num_batches_tracked")}
    assert {k: tuple(s) for k, (s, _, _) in spec.items()} == want
    with pytest.raises(ValueError, match="heads"):
        synth.vitpose_spec(C=160, heads=3)


def test_library_exports_the_new_symbols_and_validates_arguments():
    import ctypes as C
    from pmce_amd import _lib, build
    build.build()
    lib = _lib.load()
    for name in ("pmce_vit_attention_supported", "pmce_vit_attention_split_f16", "pmce_layernorm_rows_f32", "pmce_deconv4x4s2_gather_f32",
                 "pmce_vitpose_create", "pmce_vitpose_destroy", "pmce_vitpose_tensor_count", "pmce_vitpose_tensor_name",
                 "pmce_vitpose_tensor_shape", "pmce_vitpose_set_tensor", "pmce_vitpose_finalize_on", "pmce_vitpose_workspace_bytes",
                 "pmce_vitpose_forward"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert lib.pmce_vit_attention_supported(192, 1280, 16) == 1 and lib.pmce_vit_attention_supported(1, 128, 2) == 1
    assert lib.pmce_vit_attention_supported(193, 1280, 16) == 0 and lib.pmce_vit_attention_supported(192, 1280, 10) == 0
    assert lib.pmce_vit_attention_supported(0, 128, 2) == 0
    assert lib.pmce_vit_attention_split_f16(16, 16, 1, 200, 128, 2, None) == -1 and "N=200" in _lib.last_error()
    assert lib.pmce_vit_attention_split_f16(16, 16, 1, 12, 96, 2, None) == -1 and "C=96" in _lib.last_error()
    assert lib.pmce_layernorm_rows_f32(16, 4, 40, None, 0, None, 16, 16, 1e-6, 16, 0, None) == -1 and "C=40" in _lib.last_error()
    assert lib.pmce_layernorm_rows_f32(16, 4, 4096, None, 0, None, 16, 16, 1e-6, 16, 0, None) == -1 and "C=4096" in _lib.last_error()
    assert lib.pmce_deconv4x4s2_gather_f32(16, 16, 16, 1, 4, 3, 24, 0, None) == -1 and "Cout=24" in _lib.last_error()
    h = C.c_void_p()
    for args, word in (((256, 192, 1280, 32, 10, 256, 256, 17), "num_heads=10"), ((256, 192, 1290, 32, 16, 256, 256, 17), "1290"),
                       ((256, 256, 1280, 32, 16, 256, 256, 17), "256 tokens"), ((256, 192, 1280, 0, 16, 256, 256, 17), "depth"),
                       ((256, 192, 1280, 32, 16, 250, 256, 17), "250"), ((256, 192, 1280, 32, 16, 256, 256, 65), "65")):
        assert lib.pmce_vitpose_create(*args, C.byref(h)) == -1 and word in _lib.last_error(), (args, _lib.last_error())
    assert lib.pmce_vitpose_create(256, 192, 1280, 32, 16, 256, 256, 17, C.byref(h)) == 0
    n = lib.pmce_vitpose_tensor_count(h)
    names = [lib.pmce_vitpose_tensor_name(h, i).decode() for i in range(n)]
    assert n == 3 + 12 * 32 + 2 + 6 and names[0] == "backbone.pos_embed" and "backbone.blocks.31.mlp.fc2.bias" in names
    shape = (C.c_int * 4)()
    assert lib.pmce_vitpose_tensor_shape(h, names.index("keypoint_head.deconv_layers.0.weight"), shape) == 2 and tuple(shape[:2]) == (4096, 1280)
    assert lib.pmce_vitpose_tensor_shape(h, 0, shape) == 2 and tuple(shape[:2]) == (192, 1280)
    assert lib.pmce_vitpose_set_tensor(h, b"nope", 16) == -1 and "nope" in _lib.last_error()
    assert lib.pmce_vitpose_finalize_on(h, None) == -1 and "backbone.pos_embed" in _lib.last_error()     # nothing was set
    assert lib.pmce_vitpose_workspace_bytes(h, 0) == 0 and lib.pmce_vitpose_workspace_bytes(h, 257) == 0
    one, two = lib.pmce_vitpose_workspace_bytes(h, 1), lib.pmce_vitpose_workspace_bytes(h, 2)
    assert one > 0 and two == 2 * one
    assert lib.pmce_vitpose_forward(h, 16, 1, 1, 1, 1, 1, 16, None, 16, 1 << 40, None) == -1 and "not finalized" in _lib.last_error()
    lib.pmce_vitpose_destroy(h)
    with pytest.raises(ValueError, match="max_batch"):
        from pmce_amd import vitpose
        vitpose.ViTPose({}, {}, "cpu", max_batch=0)
