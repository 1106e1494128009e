"""The lifter at embed_dim 128 and 384 (heads of 16 and 48 channels) on the GPU: every row kernel, both attention kernels, the products at the
new shapes, and the whole path through the drop-in modules against the oracle - with the bounds the project holds at 256 / 512
(tests/test_gpu_ops.py, tests/test_gpu_e2e.py, tests/test_gpu_demo.py).

The row kernels keep one lane layout at every width (lane l holds channels 256 i + 4 l + [0, 4)); at 128 and 384 the last 256-channel
group is half filled and lanes 32..63 hold nothing of it: a wrong variance count, a sum over a stale register or a store past the row
shows in every case below.  The matrix-pipe attention at these widths is a kernel of its own (csrc/lifter_attention_mfma.hip: units of
512 / 768 bytes per row, part of a 32 x 32 output tile unused) around the head stage it shares with the 256 / 512 kernel; its battery is
tests/test_gpu_seq_attention.py ("lmfma"), here it keeps its fixed 5e-6."""
import numpy as np
import pytest
import torch

from conftest import cached_state_dict
from test_gpu_e2e import TIGHT_M, TOL_MM

pytestmark = pytest.mark.gpu

WIDTHS = [128, 384]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU (run with -m gpu on the GPU box)"
    return torch.device("cuda:0")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def maxabs(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).abs().max())


def rnd(name, shape, scale=1.0, seed=5):
    from pmce_amd import synth
    return T(synth.uniform_pm1(name, int(np.prod(shape)), seed).reshape(shape) * np.float32(scale))


def bits(t):
    return t.contiguous().view(torch.int32)


# ---- row kernels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [2 * 16 * 17, 51])       # 51: not a multiple of the 4 rows of a workgroup
@pytest.mark.parametrize("C", WIDTHS)
def test_ln_chain(C, rows):
    from pmce_amd import ops
    J, Tn = 17, 16
    x = rnd("ln.x", (rows, C), 2.0).to(dev())
    w1, b1 = (1 + rnd("ln.w1", (C,), 0.1)).to(dev()), rnd("ln.b1", (C,), 0.1).to(dev())
    w2, b2 = (1 + rnd("ln.w2", (C,), 0.1)).to(dev()), rnd("ln.b2", (C,), 0.1).to(dev())
    add = rnd("ln.add", (Tn, C), 0.1).to(dev())
    o1, o2 = ops.ln_chain(x, w1, b1, 1e-6, add, J, Tn, True, w2, b2, 1e-5)
    F = torch.nn.functional
    t = (torch.arange(rows, device=dev()) // J) % Tn
    r1 = F.layer_norm(x.double(), (C,), w1.double(), b1.double(), 1e-6) + add.double()[t]
    r2 = F.layer_norm(r1, (C,), w2.double(), b2.double(), 1e-5)
    e = (maxabs(o1, r1), maxabs(o2, r2))
    _, o3 = ops.ln_chain(x, None, None, 0.0, None, 1, 1, False, w2, b2, 1e-6)
    e3 = maxabs(o3, F.layer_norm(x.double(), (C,), w2.double(), b2.double(), 1e-6))
    print(f"ln_chain C={C} rows={rows}: out1 {e[0]:.2e}, out2 {e[1]:.2e}, out2 alone {e3:.2e}")
    assert e[0] < 5e-6 and e[1] < 5e-6 and e3 < 5e-6
    # out2 written pre-split for the three-product f16 GEMM: the same bits as splitting the fp32 output afterwards
    _, o2p = ops.ln_chain(x, w1, b1, 1e-6, add, J, Tn, True, w2, b2, 1e-5, out2_split=True)
    assert torch.equal(bits(o2p), bits(ops.split_rows_f16(o2)))


@pytest.mark.parametrize("BT", [37, 5000])                # one token per wavefront; wavefronts shared by a frame's tokens
@pytest.mark.parametrize("J,C", [(17, 128), (19, 384)])
def test_embed_ln_equals_embed_then_ln_chain(J, C, BT):
    from pmce_amd import ops
    pose2d = rnd("emb.p", (BT, J, 2)).to(dev())
    E = rnd("emb.E", (BT, C)).to(dev())
    Wje = rnd("emb.W", (C, 2)).to(dev())
    bje = rnd("emb.b", (C,), scale=0.1).to(dev())
    spos = rnd("emb.s", (J, C), scale=0.2).to(dev())
    w2 = (1.0 + rnd("emb.w2", (C,), scale=0.1)).to(dev())
    b2 = rnd("emb.b2", (C,), scale=0.1).to(dev())
    x_ref = ops.embed_tokens(pose2d, E, Wje, bje, spos)
    for split in (False, True):
        _, xn_ref = ops.ln_chain(x_ref, want_out1=False, w2=w2, b2=b2, eps2=1e-6, out2_split=split)
        x, xn = ops.embed_ln(pose2d, E, Wje, bje, spos, w2, b2, 1e-6, xn_split=split)
        assert torch.equal(x, x_ref), f"tokens differ (split={split})"
        assert torch.equal(bits(xn), bits(xn_ref)), f"LayerNorm output differs (split={split})"
    tok = (pose2d.double().reshape(-1, 2) @ Wje.double().T + bje.double()) + E.double().repeat_interleave(J, 0) + spos.double().repeat(BT, 1)
    ln = torch.nn.functional.layer_norm(tok, (C,), w2.double(), b2.double(), 1e-6)
    _, xn32 = ops.embed_ln(pose2d, E, Wje, bje, spos, w2, b2, 1e-6, xn_split=False)
    e = (maxabs(x, tok), maxabs(xn32, ln))
    print(f"embed_ln J={J} C={C} BT={BT}: tokens vs fp64 {e[0]:.2e}, LayerNorm vs fp64 {e[1]:.2e}")
    assert e[0] < 2e-6 and e[1] < 5e-6


@pytest.mark.parametrize("Tn", [16, 5, 23])
@pytest.mark.parametrize("C", WIDTHS)
def test_lifter_head_with_folded_post_norm(C, Tn):
    from pmce_amd import ops
    B, J = 3, 17
    x = rnd("head.x", (B * Tn * J, C), scale=2.0).to(dev())
    ntw = (1.0 + rnd("head.ntw", (C,), scale=0.1)).to(dev()); ntb = rnd("head.ntb", (C,), scale=0.1).to(dev())
    lnw = (1.0 + rnd("head.lnw", (C,), scale=0.1)).to(dev()); lnb = rnd("head.lnb", (C,), scale=0.1).to(dev())
    Wr = rnd("head.Wr", (3, C), scale=C ** -0.5).to(dev()); br = rnd("head.br", (3,), scale=0.1).to(dev())
    wf = rnd("head.wf", (Tn,), scale=0.25).to(dev()); bf = rnd("head.bf", (1,), scale=0.1).to(dev())
    y, _ = ops.ln_chain(x, ntw, ntb, 1e-6)
    two = ops.lifter_head(y, lnw, lnb, Wr, br, wf, bf, B, Tn, J)
    one = ops.lifter_head(x, lnw, lnb, Wr, br, wf, bf, B, Tn, J, pre=(ntw, ntb, 1e-6))
    assert torch.equal(one, two)
    F = torch.nn.functional
    y64 = F.layer_norm(x.double(), (C,), ntw.double(), ntb.double(), 1e-6)
    p = F.layer_norm(y64, (C,), lnw.double(), lnb.double(), 1e-5) @ Wr.double().T + br.double()
    ref = (p.reshape(B, Tn, J, 3) * wf.double()[None, :, None, None]).sum(1) + bf.double()
    e = maxabs(one, ref)
    print(f"lifter head with norm_t folded in, C={C} T={Tn}: vs fp64 {e:.2e}")
    assert e < 5e-6


@pytest.mark.parametrize("split", [False, True])
@pytest.mark.parametrize("J,C", [(17, 128), (19, 384)])
def test_window_tokens_and_mid_tokens(J, C, split):
    """pmce_window_tokens_f32 (gather + position add + LayerNorm) against fp64, and pmce_window_mid_tokens_f32 on top of it: a window whose
    mid-table row equals its frame-table row keeps its bits, the others take the mid table's row."""
    from pmce_amd import _lib, ops, streaming
    lib = _lib.load()
    P = _lib.ptr
    L, Tn = 21, 16
    win_np = streaming.demo_window_list(L).astype(np.int32)
    W = len(win_np)
    win = T(win_np).to(dev())
    x0 = rnd("win.x0", (L, J, C), 2.0).to(dev())
    x0_mid = x0.clone()
    changed = torch.arange(L, device=dev()) % 3 == 1
    x0_mid[changed] += 0.5
    tpos = rnd("win.tpos", (Tn, C), 0.1).to(dev())
    w2, b2 = (1 + rnd("win.w2", (C,), 0.1)).to(dev()), rnd("win.b2", (C,), 0.1).to(dev())
    X = torch.empty(W * Tn * J, C, device=dev())
    XN = torch.empty_like(X)
    _lib.check(lib.pmce_window_tokens_f32(P(x0), P(win), P(tpos), P(w2), P(b2), 1e-6, P(X), P(XN), W, L, Tn, J, C, int(split),
                                          _lib.current_stream()), "window_tokens")
    fr = np.stack([np.full(Tn, s) if s == e else np.arange(s, s + Tn) for s, e in win_np]).clip(0, L - 1)       # [W, T]
    fr = T(fr).to(dev())
    ref = x0.double()[fr] + tpos.double()[None, :, None, :]                                                   # [W, T, J, C]
    refn = torch.nn.functional.layer_norm(ref, (C,), w2.double(), b2.double(), 1e-6)
    XN32 = ops.unsplit_rows_f16(XN).reshape(W, Tn, J, C) if split else XN.reshape(W, Tn, J, C)
    e = (maxabs(X.reshape(W, Tn, J, C), ref), maxabs(XN32, refn))
    print(f"window_tokens J={J} C={C} split={split}: X {e[0]:.2e}, XN {e[1]:.2e}")
    assert e[0] < 5e-6 and e[1] < 5e-6
    # the same rows through ln_chain on the gathered table: bit for bit
    g = x0[fr].reshape(W * Tn * J, C).contiguous()
    o1, o2 = ops.ln_chain(g, None, None, 0.0, tpos, J, Tn, True, w2, b2, 1e-6, out2_split=split)
    assert torch.equal(X, o1) and torch.equal(bits(XN), bits(o2))
    X0, XN0 = X.clone(), XN.clone()
    t_mid = Tn // 2
    _lib.check(lib.pmce_window_mid_tokens_f32(P(x0_mid), P(win), P(tpos), P(w2), P(b2), 1e-6, P(X), P(XN), W, L, Tn, J, C, t_mid, int(split),
                                              _lib.current_stream()), "window_mid_tokens")
    Xv, X0v = X.reshape(W, Tn, J, C), X0.reshape(W, Tn, J, C)
    XNv, XN0v = XN.reshape(W, Tn, J, C), XN0.reshape(W, Tn, J, C)
    midf = fr[:, t_mid]
    keep = ~changed[midf]
    assert bool(keep.any()) and bool((~keep).any())
    other_t = [t for t in range(Tn) if t != t_mid]
    assert torch.equal(Xv[:, other_t], X0v[:, other_t]) and torch.equal(bits(XNv[:, other_t]), bits(XN0v[:, other_t]))
    assert torch.equal(Xv[keep, t_mid], X0v[keep, t_mid]) and torch.equal(bits(XNv[keep, t_mid]), bits(XN0v[keep, t_mid]))
    refm = x0_mid.double()[midf] + tpos.double()[t_mid]                                                       # [W, J, C]
    refmn = torch.nn.functional.layer_norm(refm, (C,), w2.double(), b2.double(), 1e-6)
    XNm = ops.unsplit_rows_f16(XN).reshape(W, Tn, J, C)[:, t_mid] if split else XNv[:, t_mid]
    em = (maxabs(Xv[:, t_mid], refm), maxabs(XNm, refmn))
    print(f"   window_mid_tokens: X {em[0]:.2e}, XN {em[1]:.2e}")
    assert em[0] < 5e-6 and em[1] < 5e-6


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
def attention_fp64(x64, B, Tn, J, C, seq_first):
    """timm Attention on [B*Tn*J, 3C] float64, tokens laid out [b, t, j]; sequences over j ("s") or over t ("t")."""
    H = 8
    hd = C // H
    M = B * Tn * J
    x = x64.reshape(B, Tn, J, 3, H, hd)
    x = x if seq_first == "s" else x.permute(0, 2, 1, 3, 4, 5)
    q, k, v = x[..., 0, :, :], x[..., 1, :, :], x[..., 2, :, :]
    q, k, v = (z.permute(0, 1, 3, 2, 4) for z in (q, k, v))
    a = ((q @ k.transpose(-2, -1)) * hd ** -0.5).softmax(-1) @ v
    a = a.permute(0, 1, 3, 2, 4).reshape(*a.shape[:2], a.shape[3], C)
    return (a if seq_first == "s" else a.permute(0, 2, 1, 3)).reshape(M, C)


def layouts(B, Tn, J, C):
    return (("spatial", (B * Tn, J, C, 0, J, 0, 1)), ("temporal", (B * J, Tn, C, J, 1, Tn * J, J)))


@pytest.mark.parametrize("J", [17, 19])
@pytest.mark.parametrize("C", WIDTHS)
def test_seq_attention_vector_pipe(C, J):
    from pmce_amd import ops
    B, Tn = 2, 16
    qkv = rnd("attn.qkv", (B * Tn * J, 3 * C)).to(dev())
    for name, args in layouts(B, Tn, J, C):
        out = ops.lifter_attention(qkv, *args)
        e = maxabs(out, attention_fp64(qkv.double(), B, Tn, J, C, name[0]))
        print(f"seq_attention C={C} J={J} {name}: {e:.2e}")
        assert e < 5e-6
        planes = ops.lifter_attention(qkv, *args, out_split=True)
        assert torch.equal(bits(planes), bits(ops.split_rows_f16(out)))


@pytest.mark.parametrize("C", WIDTHS)
def test_seq_attention_of_one_token_returns_v(C):
    """N = 1: softmax of one score is 1, the result is v bit for bit (at 256 it once was an ulp away: test_gpu_seq_attention.py)."""
    from pmce_amd import ops
    M = 70
    qkv = (rnd("attn.one", (M, 3 * C)) * 3.0).to(dev())
    out = ops.lifter_attention(qkv, M, 1, C, 0, 1, 0, 1)
    assert torch.equal(out, qkv[:, 2 * C:])


@pytest.mark.parametrize("C,J,B", [(128, 17, 2), (384, 17, 2), (128, 19, 1), (384, 19, 3), (384, 17, 37)])
def test_lifter_attention_split_f16(C, J, B):
    """The matrix-pipe attention at heads of 16 and 48 channels on the inputs of test_gpu_ops.py::test_seq_attention_split_f16 (x 1.7: a peaked
    softmax) against the fp64 attention of the values the (hi, lo) planes of q, k, v hold: within 5e-6, a fixed bound stated for these head
    sizes.  The analytic bound, the exact cases, repeatability, a sequence alone against its rows in a launch and the persistent workgroups
    are the "lmfma" instances of tests/test_gpu_seq_attention.py."""
    from pmce_amd import ops
    Tn = 16
    M = B * Tn * J
    qkv = (rnd("attn.qkv", (M, 3 * C)) * 1.7).to(dev())
    exact = ops.unsplit_rows_f16(ops.split_rows_f16(qkv))                     # float64 [M, 3C]: the values the planes hold
    assert (exact - qkv.double()).abs().max().item() < 1e-5
    for name, args in layouts(B, Tn, J, C):
        want = attention_fp64(exact, B, Tn, J, C, name[0])
        got = ops.unsplit_rows_f16(ops.lifter_attention_split(qkv, *args))
        e = (got - want).abs().max().item()
        print(f"lifter_attention_split_f16 C={C} J={J} B={B} {name}: {e:.2e}, |out| max {want.abs().max().item():.2f}")
        assert bool(torch.isfinite(got).all())
        assert e < 5e-6


@pytest.mark.parametrize("C,J", [(256, 17), (512, 19), (512, 16)])
def test_lifter_attention_forwards_the_existing_widths(C, J):
    from pmce_amd import ops
    B, Tn = 2, 16
    qkv = (rnd("attn.qkv", (B * Tn * J, 3 * C)) * 1.7).to(dev())
    for name, args in layouts(B, Tn, J, C):
        assert torch.equal(bits(ops.lifter_attention_split(qkv, *args)), bits(ops.seq_attention_split(qkv, *args)))
        for split in (False, True):
            assert torch.equal(bits(ops.lifter_attention(qkv, *args, out_split=split)), bits(ops.seq_attention(qkv, *args, out_split=split)))


# ---- products at the lifter's new shapes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", [-1, 0, 1, 2])
@pytest.mark.parametrize("C", WIDTHS)
@pytest.mark.parametrize("which", ["qkv", "proj", "fc1", "fc2"])
def test_products_at_the_new_shapes(which, C, tile):
    """qkv, proj (+ residual), fc1 (GELU, pre-split out) and fc2 (+ residual) of a lifter block at M = 2 * 16 * 17, by the recipe of
    test_gpu_ops.py::test_gemm_nt_split: the three-product f16 form against the fp64 product next to the fp32 pipe's own error, every forced
    tile configuration, fp32 and pre-split A."""
    from pmce_amd import _lib, ops
    M = 2 * 16 * 17
    N, K, act, res = {"qkv": (3 * C, C, 0, False), "proj": (C, C, 0, True), "fc1": (2 * C, C, 1, False), "fc2": (C, 2 * C, 0, True)}[which]
    lib = _lib.load()
    A = rnd("gemm.A", (M, K)).to(dev())
    A[::5] *= 1e-3
    W = rnd("gemm.W", (N, K), scale=K ** -0.5).to(dev())
    b = rnd("gemm.b", (N,)).to(dev())
    R = rnd("gemm.R", (M, N)).to(dev()) if res else None
    Wp, ws = ops.pack_split_f16(W)
    lib.pmce_gemm_split_set_tuning(tile)
    try:
        out = ops.gemm_nt_split(A, Wp, ws, b, R, act)
        outp = ops.gemm_nt_split(ops.split_rows_f16(A), Wp, ws, b, R, act, a_packed=True)
        outc = ops.gemm_nt_split(ops.split_rows_f16(A), Wp, ws, b, R, act, a_packed=True, c_packed=True) if which == "fc1" else None
    finally:
        lib.pmce_gemm_split_set_tuning(-1)
    out32 = ops.gemm_nt(A, W, b, R, act)
    ref = A.double() @ W.double().t() + b.double()
    if act:
        ref = torch.nn.functional.gelu(ref)
    if res:
        ref = ref + R.double()
    e, e32 = maxabs(out, ref), maxabs(out32, ref)
    print(f"{which} C={C} ({M}x{N}x{K}) tile={tile}: max-abs {e:.2e} (fp32 pipe {e32:.2e})")
    assert torch.equal(out, outp)
    assert e < 2e-5 and e <= 1.5 * e32 + 1e-7
    if outc is not None:                  # fc1's pre-split result (the operand of fc2): the fp32 result's bits, split
        assert torch.equal(bits(outc), bits(ops.split_rows_f16(out)))


# ---- the whole path ------------------------------------------------------------------------------------------------------------------------
_MODELS = {}


def get_model(J, C, regressor="h36m"):
    from pmce_amd import assets, models
    key = (J, C, regressor)
    if key not in _MODELS:
        _MODELS.clear()
        torch.cuda.empty_cache()
        m = models.PMCE.get_model(J, C, 3)
        m.load_state_dict(cached_state_dict(J, C))
        m.set_j_regressor(assets.load_j_regressor(regressor))
        _MODELS[key] = m.to(dev())
    return _MODELS[key]


def set_mode(model, mode):
    if mode == "f32":
        model.set_gemm_mode("f32")
    else:
        model.set_gemm_mode("split_f16", min_batch=1)


@pytest.mark.parametrize("mode", ["split_f16", "f32"])
@pytest.mark.parametrize("J,C", [(17, 128), (19, 128), (17, 384), (19, 384)])
def test_forward_matches_oracle(J, C, mode):
    """models.PMCE.get_model(J, C, 3), B = 3, against the oracle, split-f16 at every batch size and on the fp32 pipe.  The oracle's own
    fp32 noise on these inputs (its fp32 evaluation against its fp64 evaluation, on the CPU): mesh 1.1e-6 m at C = 128 and 1.1e-6 m at
    C = 384 (pose 6.4e-7 .. 7.4e-7 m, pose3d 3.1e-4 .. 5.0e-4 mm) - a fiftieth of TIGHT_M = 5e-5 m and a fortieth of TOL_MM = 2e-2 mm, as
    at 256 (~2e-6 m)."""
    from oracle import pmce_oracle as O
    from pmce_amd import synth
    B = 3
    model = get_model(J, C)
    sd = cached_state_dict(J, C)
    pose2d, img_feat = synth.make_inputs(B, J, 77)
    set_mode(model, mode)
    try:
        mesh, pose, pose3d = model(T(pose2d).to(dev()), T(img_feat).to(dev()))
        cm, cp, cl, cpred = model.forward_with_joints(T(pose2d).to(dev()), T(img_feat).to(dev()))
        torch.cuda.synchronize()
    finally:
        model.set_gemm_mode(None)
    with torch.no_grad():
        rm, rp, rl = O.pmce_forward(sd, T(pose2d), T(img_feat), model.vj_relation)
    e = (maxabs(mesh, rm), maxabs(pose, rp), maxabs(pose3d, rl))
    print(f"J={J} C={C} {mode} vs oracle: mesh %.2e m, pose %.2e m, pose3d %.2e mm" % e)
    assert e[0] < TIGHT_M and e[1] < TIGHT_M and e[2] < TOL_MM
    assert torch.equal(cm, mesh) and torch.equal(cl, pose3d) and bool(torch.isfinite(cpred).all())


def test_lifter_alone_and_depth_one():
    from oracle import pmce_oracle as O
    from pmce_amd import assets, models, synth
    J, C, B = 17, 384, 3
    sd = synth.make_state_dict(synth.lifter_spec(J, C, 3), seed=321)
    lifter = models.PoseEstimation.get_model(J, C, 3)
    lifter.load_state_dict(sd)
    lifter = lifter.to(dev())
    pose2d, img_feat = synth.make_inputs(B, J, 8)
    out = lifter(T(pose2d).to(dev()), T(img_feat).to(dev()))
    with torch.no_grad():
        ref = O.lifter_forward(sd, T(pose2d), T(img_feat), 3, "")
    e = maxabs(out, ref)
    print(f"PoseEstimation.get_model(17, 384, 3) vs oracle: pose3d {e:.2e} mm")
    assert e < TOL_MM
    J, C, depth = 17, 128, 1
    sd = synth.make_state_dict(synth.pmce_spec(J, C, depth), seed=321)
    model = models.PMCE.get_model(J, C, depth)
    model.load_state_dict(sd)
    model.set_j_regressor(assets.load_j_regressor("h36m"))
    model = model.to(dev())
    mesh, pose, pose3d = model(T(pose2d[:2]).to(dev()), T(img_feat[:2]).to(dev()))
    with torch.no_grad():
        rm, rp, rl = O.pmce_forward(sd, T(pose2d[:2]), T(img_feat[:2]), model.vj_relation, depth=depth)
    e = (maxabs(mesh, rm), maxabs(pose, rp), maxabs(pose3d, rl))
    print("depth 1, C = 128 vs oracle: mesh %.2e m, pose %.2e m, pose3d %.2e mm" % e)
    assert e[0] < TIGHT_M and e[1] < TIGHT_M and e[2] < TOL_MM


def test_a_clip_does_not_depend_on_its_batch():
    """C = 384 in split mode: clip 0 of B = 1, 3 and 40 is the same bits (the products pick other tiles, the attention other grids)."""
    from pmce_amd import synth
    J, C = 17, 384
    model = get_model(J, C)
    pose2d, img_feat = synth.make_inputs(40, J, 11)
    p, f = T(pose2d).to(dev()), T(img_feat).to(dev())
    model.set_gemm_mode("split_f16", min_batch=1)
    try:
        outs = [tuple(o[:1].clone() for o in model(p[:b], f[:b])) for b in (1, 3, 40)]
        torch.cuda.synchronize()
    finally:
        model.set_gemm_mode(None)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.equal(a, b)


@pytest.mark.parametrize("J,C,L", [(17, 384, 40), (19, 128, 23)])
def test_streaming_matches_oracle(J, C, L):
    """tests/test_gpu_e2e.py::test_streaming_matches_oracle's recipe at the new widths: one window per frame of an L-frame sequence through
    the frame-reuse path against the oracle forward of the same windows assembled on the host."""
    from oracle import pmce_oracle as O
    from pmce_amd import streaming, synth
    model = get_model(J, C)
    sd = cached_state_dict(J, C)
    nclip = (L + 15) // 16
    p_np, f_np = synth.make_inputs(nclip, J, 90 + J)
    pose_fr, feat_fr = p_np.reshape(-1, J, 2)[:L], f_np.reshape(-1, 2048)[:L]
    win = streaming.demo_window_list(L)
    wp = np.stack([pose_fr[[s] * 16] if s == e else pose_fr[s:e + 1] for s, e in win])
    wf = np.stack([feat_fr[[s] * 16] if s == e else feat_fr[s:e + 1] for s, e in win])
    with torch.no_grad():
        rm, rp, rl = O.pmce_forward(sd, T(wp), T(wf), model.vj_relation)
    cache = streaming.precompute_frames(model, T(pose_fr).to(dev()), T(feat_fr).to(dev()))
    mesh, pose, pose3d, pred = streaming.stream_forward_cached(model, cache, windows=win, batch=24, with_joints=True, lanes=2)
    e = (maxabs(mesh, rm), maxabs(pose, rp), maxabs(pose3d, rl))
    print(f"streamed J={J} C={C} L={L} vs oracle: mesh %.2e m, pose %.2e m, pose3d %.2e mm" % e)
    assert e[0] < TIGHT_M and e[1] < TIGHT_M and e[2] < TOL_MM


@pytest.mark.parametrize("middle_frame", ["reference", "clean"])
def test_demo_tracklet_at_width_128(middle_frame):
    """demo.run_tracklet on 30 frames at C = 128, with the demo's middle-frame override ("reference") and without ("clean"): finite, and the
    frame-reuse path equals the assembled-window forward (reuse=False) to the bounds of tests/test_gpu_demo.py."""
    import demo_ref as DR
    from pmce_amd import demo
    model = get_model(19, 128, "coco")
    kp, wh = DR.tracklet(0)
    kp, feat = T(kp[:30]).to(dev()), T(DR.features(0)[:30]).to(dev())
    init = T(np.array([[0.3, 0.1, 0.2]], dtype=np.float32)).to(dev())
    out = demo.run_tracklet(model, kp, feat, wh, batch=16, init=init, middle_frame=middle_frame)
    unc = demo.run_tracklet(model, kp, feat, wh, batch=16, init=init, middle_frame=middle_frame, reuse=False)
    torch.cuda.synchronize()
    assert tuple(out["mesh"].shape) == (30, 6890, 3)
    for key in ("mesh", "joints_mm", "pred_cam", "orig_cam", "loss"):
        assert bool(torch.isfinite(out[key]).all()), key
    u = (maxabs(out["mesh"], unc["mesh"]), maxabs(out["joints_mm"], unc["joints_mm"]))
    print(f"run_tracklet C=128 {middle_frame}: cached vs assembled windows mesh {u[0]:.2e} m, joints {u[1]:.2e} mm")
    assert u[0] < TIGHT_M and u[1] < 1000 * TIGHT_M


def test_bench_widths_writes_its_schema(tmp_path):
    """scripts/bench_widths.py at a batch of 4 with one pass: the layout of the JSON it writes (no time is asserted)."""
    import json
    import os.path as osp
    import subprocess
    import sys
    from conftest import REPO
    out = tmp_path / "widths.json"
    r = subprocess.run([sys.executable, osp.join(REPO, "scripts", "bench_widths.py"), "--batch", "4", "--reps", "1", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(out.read_text())
    assert res["J"] == 17 and res["batch"] == 4 and res["reps"] == 1 and isinstance(res["forward_ms_monotonic_in_width"], bool)
    assert sorted(res["widths"]) == ["128", "256", "384", "512"] and sorted(res["matrix_pipe_attention_faster"]) == ["128", "256", "384", "512"]
    for w in res["widths"].values():
        assert w["forward_ms_median"] > 0 and w["forward_ms_min"] > 0 and w["clips_per_s"] > 0 and isinstance(w["sclk_after"], str)
        assert sorted(w["classes"]) == ["gemm_lifter", "ln_chain", "seq_attention"]
        for c in w["classes"].values():
            assert c["launches_per_forward"] > 0 and c["us_per_launch_median"] > 0 and c["ms_per_forward_median"] > 0
        assert sorted(w["attention"]) == ["spatial", "temporal"]
        for a in w["attention"].values():
            assert a["matrix_pipe_us_median"] > 0 and a["vector_pipe_us_median"] > 0 and a["vector_over_matrix"] > 0


def test_graphed_and_pipelined_forward_at_width_384():
    """models.PMCE.graphed(1) (the forward replayed from a captured graph) and models.PMCE.pipeline() (batches in flight on shared weights) at
    C = 384: the same bits as the direct call, by the recipes of tests/test_gpu_e2e.py."""
    from pmce_amd import synth
    J, C = 17, 384
    model = get_model(J, C)
    gf = model.graphed(1)
    for seed in (5, 6):
        p, f = (T(a).to(dev()) for a in synth.make_inputs(1, J, seed))
        ref = [t.clone() for t in model.forward_with_joints(p, f)]
        got = gf(p, f)
        torch.cuda.synchronize()
        for a, b in zip(ref, got):
            assert torch.equal(a, b)
    batches = []
    for i, B in enumerate((5, 3, 8, 1)):
        p, f = synth.make_inputs(B, J, 700 + i)
        batches.append((T(p).to(dev()), T(f).to(dev())))
    direct = [tuple(t.clone() for t in model.forward_with_joints(p, f)) for p, f in batches]
    pipe = model.pipeline(depth=2)
    tickets = [pipe.submit(p, f) for p, f in batches]
    for d, t in zip(direct, tickets):
        for a, b in zip(d, t.result()):
            assert torch.equal(a, b)
    pipe.synchronize()
