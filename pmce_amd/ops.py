"""Per-operator Python wrappers over the C ABI (include/pmce_hip.h).  Used by the parity tests and by callers that
want a single stage; the whole-path modules in pmce_amd/models call pmce_forward instead.  All tensors are
contiguous fp32 CUDA tensors; weights are passed the way the reference's state_dict stores them."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .packing import N_ADA

P = _lib.ptr


def _st():
    return _lib.current_stream()


def _c(t):
    return t.to(torch.float32).contiguous()


def gemm_nt(A, W, bias=None, residual=None, act=0, out=None):
    """out = act(A @ W^T + bias) + residual  (nn.Linear)."""
    lib = _lib.load()
    A, W = _c(A), _c(W)
    M, K = A.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    _lib.check(lib.pmce_gemm_nt_f32(P(A), P(W), P(bias), P(residual), P(out), M, N, K, K, K, N, act, 0, 0, 0, 0, 0, 0, 1,
                                    0, 0, 0, 0, _st()), "gemm_nt")
    return out


def pack_split_f16(W):
    """W[N,K] fp32 -> (Wp[N,K] storage of the f16 hi/lo planes, wscale[N] = 2^-s per output row) for :func:`gemm_nt_split`."""
    lib = _lib.load()
    W = _c(W)
    N, K = W.shape
    Wp = torch.empty(N, K, device=W.device, dtype=torch.float32)
    wscale = torch.empty(N, device=W.device, dtype=torch.float32)
    _lib.check(lib.pmce_gemm_pack_split_f16(P(W), N, K, K, P(Wp), P(wscale), 0, _st()), "gemm_pack_split_f16")
    return Wp, wscale


def pack_split_f16_blk(W):
    """The same planes in the blocked layout [ceil(N/64)][K/16][64][16 hi | 16 lo] (what the model packs); -> (Wblk, wscale, N)."""
    lib = _lib.load()
    W = _c(W)
    N, K = W.shape
    Np = (N + 63) // 64 * 64
    Wp = torch.zeros(Np, K, device=W.device, dtype=torch.float32)
    ws = torch.empty(N, device=W.device, dtype=torch.float32)
    _lib.check(lib.pmce_gemm_pack_split_f16(P(W), N, K, K, P(Wp), P(ws), 1, _st()), "gemm_pack_split_f16")
    return Wp, ws, N


def _gemm_nt_split(A, Wp, blocked, wscale, N, bias=None, residual=None, act=0, a_packed=False, c_packed=False, rscale=None, rowmap=None, out=None):
    """pmce_gemm_nt_split_f16: every form of the three-product GEMM, on a row-major or a blocked weight."""
    lib = _lib.load()
    M, K = A.shape
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32)
    cd, lo, hi = rowmap if rowmap else (0, 0, 0)
    _lib.check(lib.pmce_gemm_nt_split_f16(P(A), P(rscale), P(Wp), 1 if blocked else 0, P(wscale), P(bias), P(residual), P(out), M, N, K, K, N, act,
                                          1 if a_packed else 0, 1 if c_packed else 0, cd, lo, hi, _st()), "gemm_nt_split")
    return out


def gemm_nt_split_blk(A, Wblk, wscale, N, bias=None, residual=None, act=0, a_packed=False, c_packed=False, rscale=None, rowmap=None, out=None):
    """Every form of the three-product GEMM on a blocked weight."""
    return _gemm_nt_split(A, Wblk, True, wscale, N, bias, residual, act, a_packed, c_packed, rscale, rowmap, out)


def gemm_nt_split_ln(Ap, Wp, wscale, bias, residual, ln1=None, ln2=None, blocked=True, want_out1=True):
    """pmce_gemm_nt_split_f16_ln: x = Ap W^T + bias + residual (N = 256); y1 = LN(x; ln1) or x; returns (y1 fp32 or None,
    LN(y1; ln2) pre-split or None).  ln1 / ln2 = (weight, bias, eps)."""
    lib = _lib.load()
    M, K = Ap.shape
    out1 = torch.empty(M, 256, device=Ap.device) if want_out1 else None
    out2 = torch.empty(M, 256, device=Ap.device) if ln2 is not None else None
    w1, b1, e1 = (_c(ln1[0]), _c(ln1[1]), float(ln1[2])) if ln1 is not None else (None, None, 0.0)
    w2, b2, e2 = (_c(ln2[0]), _c(ln2[1]), float(ln2[2])) if ln2 is not None else (None, None, 0.0)
    _lib.check(lib.pmce_gemm_nt_split_f16_ln(P(Ap), P(Wp), 1 if blocked else 0, P(wscale), P(bias), P(residual), M, K, P(w1), P(b1), e1, P(out1),
                                             P(w2), P(b2), e2, P(out2), _st()), "gemm_nt_split_ln")
    return out1, out2


def split_rows_f16(A):
    """A[M,K] fp32 -> the packed (hi | lo*2^11) f16 planes, as an [M,K] float32-typed buffer."""
    lib = _lib.load()
    A = _c(A)
    M, K = A.shape
    Ap = torch.empty(M, K, device=A.device, dtype=torch.float32)
    _lib.check(lib.pmce_split_rows_f16(P(A), M, K, K, P(Ap), _st()), "split_rows_f16")
    return Ap


def gemm_nt_split(A, Wp, wscale, bias=None, residual=None, act=0, out=None, a_packed=False, c_packed=False):
    """gemm_nt on the f16 matrix pipe (three-product split, fp32 accumulate): fp32 in, fp32 out, fp32 accuracy.  Row-major weight."""
    return _gemm_nt_split(_c(A), Wp, False, wscale, Wp.shape[0], bias, residual, act, a_packed, c_packed, out=out)


def split_rows_scaled_f16(A):
    """fp32 rows of any finite magnitude -> (planes of A[m] * 2^-e(m) in the packed-A layout, rscale[m] = 2^e(m))."""
    lib = _lib.load()
    A = _c(A)
    M, K = A.shape
    Ap = torch.empty(M, K, device=A.device, dtype=torch.float32)
    rs = torch.empty(M, device=A.device, dtype=torch.float32)
    _lib.check(lib.pmce_split_rows_scaled_f16(P(A), M, K, K, P(Ap), P(rs), _st()), "split_rows_scaled_f16")
    return Ap, rs


def gemm_nt_split_rs(Ap, rscale, Wp, wscale, bias=None, out=None, rowmap=None):
    """The three-product f16 GEMM on a row-scaled packed A (raw inputs: img_feat) and a row-major weight.  rowmap = (c_div, c_lo, c_hi) maps
    output rows.  K >= 128 (include/pmce_hip.h at pmce_gemm_nt_split_f16)."""
    return _gemm_nt_split(Ap, Wp, False, wscale, Wp.shape[0], bias, a_packed=True, rscale=rscale, rowmap=rowmap, out=out)


def gru_step_split(gi, whh, bhh, h_prev, blocked=True):
    """One GRU time step of ONE direction in the three-product f16 form (nn.GRU gate order r, z, n; CoevoDecoder.py:216-221): gi [B, 3H] =
    W_ih x + b_ih, whh [3H, H], bhh [3H], h_prev [B, H] or None (h = 0) -> h' [B, H].  B <= 64 runs the small-batch kernel, larger batches
    gru_step_v2 - same numbers, bit for bit."""
    lib = _lib.load()
    gi, whh, bhh = _c(gi), _c(whh), _c(bhh)
    B, H = gi.shape[0], whh.shape[1]
    if blocked:     # the layout the model packs W_hh in
        Wp, wscale, _ = pack_split_f16_blk(whh)
    else:
        Wp, wscale = pack_split_f16(whh)
    hp = None if h_prev is None else _c(h_prev)
    out = torch.empty(B, H, device=gi.device, dtype=torch.float32)
    _lib.check(lib.pmce_gru_step_split_f32(P(gi), None, P(Wp), None, P(wscale), P(bhh), None, P(hp), None, P(out), None, 3 * H, H, B, H, 1,
                                           1 if blocked else 0, _st()), "gru_step_split")
    return out


def _row_view(t, cols, what):
    """(device pointer, row stride in floats) of a 2-D fp32 device view whose last dimension is contiguous (rows may be strided)."""
    if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape[1] == cols and t.stride(1) == 1):
        raise ValueError(f"gru_step: {what} must be an fp32 device view [B, {cols}] with a contiguous last dimension")
    if t.data_ptr() % 16 or (t.shape[0] > 1 and t.stride(0) % 4):
        raise ValueError(f"gru_step: {what} rows must start on 16-byte boundaries (the kernels fetch h in 16-byte pieces)")
    return C.c_void_p(t.data_ptr()), t.stride(0) if t.shape[0] > 1 else None


def gru_step(gi, whh, bhh, h_prev, out, form="split", blocked=True, backward_only=False):
    """One GRU time step through pmce_gru_step_f32 (form="f32") or pmce_gru_step_split_f32 (form="split"), in every shape model.cpp's
    gru_layer calls them.  whh / bhh: one [3H, H] / [3H] tensor per direction (a list of one or two).  gi / h_prev / out: one 2-D view per
    direction that runs ([B, 3H], [B, H], [B, H]; rows may be strided - a column block of a wider buffer -, the last dimension is
    contiguous); h_prev, or either of its entries, may be None (h = 0).  The row strides come from the views: gi's and h_prev's / out's
    must agree between the directions (and h_prev's with out's: the C entry takes ONE h_rs).  Writes `out` in place and returns it.

    Two directions, split form: the stacked [6H, H] weight is packed in ONE pmce_gemm_pack_split_f16 call as the model packs it; direction 1
    is that buffer + 3H * H floats and reads the second half of the one [6H] scale table.

    backward_only (with two directions' weights): gi / h_prev / out are direction 1's alone and the call is ndir = 1 on direction 1's rows of
    the stacked weight (split form: whh0p = packed + 3H * H floats, wscale + 3H) - gru_layer's backward-only branch."""
    lib = _lib.load()
    if form not in ("f32", "split"):
        raise ValueError("gru_step: form must be 'f32' or 'split'")
    whh, bhh = [_c(w) for w in whh], [_c(b) for b in bhh]
    nw = len(whh)
    if nw not in (1, 2) or len(bhh) != nw:
        raise ValueError("gru_step: one or two directions")
    if backward_only and nw != 2:
        raise ValueError("gru_step: backward_only needs both directions' weights")
    H = whh[0].shape[1]
    if any(tuple(w.shape) != (3 * H, H) for w in whh) or any(tuple(b.shape) != (3 * H,) for b in bhh):
        raise ValueError("gru_step: whh must be [3H, H] and bhh [3H] per direction")
    ndir = 1 if backward_only else nw
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v]      # noqa: E731
    gi, out = as_list(gi), as_list(out)
    h_prev = [None] * ndir if h_prev is None else as_list(h_prev)
    if not (len(gi) == len(out) == len(h_prev) == ndir):
        raise ValueError(f"gru_step: gi, h_prev and out need one view per running direction ({ndir})")
    B = gi[0].shape[0]
    gp, hp, op, gi_rs, h_rs = [], [], [], set(), set()
    for d in range(ndir):
        if gi[d].shape[0] != B or out[d].shape[0] != B or (h_prev[d] is not None and h_prev[d].shape[0] != B):
            raise ValueError("gru_step: every view has B rows")
        p, s = _row_view(gi[d], 3 * H, "gi")
        gp.append(p); gi_rs.add(s)
        p, s = _row_view(out[d], H, "out")
        op.append(p); h_rs.add(s)
        if h_prev[d] is None:
            hp.append(None)
        else:
            p, s = _row_view(h_prev[d], H, "h_prev")
            hp.append(p); h_rs.add(s)
    gi_rs.discard(None); h_rs.discard(None)           # (a single row has no stride of its own)
    if len(gi_rs) > 1 or len(h_rs) > 1:
        raise ValueError(f"gru_step: the directions' row strides differ (gi {sorted(gi_rs)}, h_prev / out {sorted(h_rs)})")
    gi_rs = gi_rs.pop() if gi_rs else 3 * H
    h_rs = h_rs.pop() if h_rs else H
    gp, hp, op = (v + [None] * (2 - ndir) for v in (gp, hp, op))
    fp = lambda t, off: C.c_void_p(t.data_ptr() + 4 * off)                    # noqa: E731
    b0, b1 = (bhh[1], None) if backward_only else (bhh[0], bhh[1] if nw == 2 else None)
    if form == "f32":
        w0, w1 = (whh[1], None) if backward_only else (whh[0], whh[1] if nw == 2 else None)
        _lib.check(lib.pmce_gru_step_f32(gp[0], gp[1], P(w0), P(w1), P(b0), P(b1), hp[0], hp[1], op[0], op[1], gi_rs, h_rs, B, H, ndir, _st()),
                   "gru_step_f32")
        return out if ndir == 2 else out[0]
    W = torch.cat(whh, 0) if nw == 2 else whh[0]
    if blocked:
        Wp, wscale, _ = pack_split_f16_blk(W)
    else:
        Wp, wscale = pack_split_f16(W)
    if backward_only:
        w0, w1, sc = fp(Wp, 3 * H * H), None, fp(wscale, 3 * H)
    else:
        w0, w1, sc = P(Wp), (fp(Wp, 3 * H * H) if nw == 2 else None), P(wscale)
    _lib.check(lib.pmce_gru_step_split_f32(gp[0], gp[1], w0, w1, sc, P(b0), P(b1), hp[0], hp[1], op[0], op[1], gi_rs, h_rs, B, H, ndir,
                                           1 if blocked else 0, _st()), "gru_step_split")
    return out if ndir == 2 else out[0]


def f16_rows(buf):
    """The plain f16 rows that form 2 of a row kernel or an attention (``out2_split`` / ``xn_split`` / ``out_split`` / ``out_form`` = 2) left in
    the first half of an fp32-typed [rows, C] buffer: a float16 [rows, C] view of them (the A operand of pmce_gemm_nt_f16)."""
    rows, Cc = buf.shape
    return buf.contiguous().view(torch.float16).reshape(-1)[:rows * Cc].view(rows, Cc)


def ln_chain(x, w1=None, b1=None, eps1=1e-6, add=None, add_div=1, add_mod=1, want_out1=True, w2=None, b2=None, eps2=1e-6,
             out2_split=False):
    """out2_split (and xn_split / out_split of the wrappers below): False / 0 fp32, True / 1 pre-split planes, 2 plain f16 rows
    (:func:`f16_rows` views them)."""
    lib = _lib.load()
    x = _c(x)
    rows, Cc = x.shape
    out1 = torch.empty_like(x) if want_out1 else None
    out2 = torch.empty_like(x) if w2 is not None else None
    _lib.check(lib.pmce_ln_chain_f32(P(x), rows, Cc, P(w1), P(b1), eps1, P(add), add_div, add_mod, P(out1), P(w2), P(b2), eps2,
                                     P(out2), int(out2_split), _st()), "ln_chain")
    return out1, out2


def embed_tokens(pose2d, E, Wje, bje, spos):
    """Token embedding (PoseEstimation.py:78-81): pose2d [BT, J, 2], E = imgfeat_embed(img_feat) [BT, C] -> tokens [BT * J, C]."""
    lib = _lib.load()
    BT, J, _ = pose2d.shape
    Cc = E.shape[1]
    x = torch.empty(BT * J, Cc, device=E.device, dtype=torch.float32)
    _lib.check(lib.pmce_embed_tokens_f32(P(_c(pose2d)), P(_c(E)), P(_c(Wje)), P(_c(bje)), P(_c(spos)), P(x), BT * J, J, Cc, _st()), "embed_tokens")
    return x


def embed_ln(pose2d, E, Wje, bje, spos, w2, b2, eps2=1e-6, xn_split=False):
    """embed_tokens + LayerNorm(w2, b2) of every row in one launch: (tokens, their LayerNorm - pre-split planes when xn_split)."""
    lib = _lib.load()
    BT, J, _ = pose2d.shape
    Cc = E.shape[1]
    x = torch.empty(BT * J, Cc, device=E.device, dtype=torch.float32)
    xn = torch.empty_like(x)
    _lib.check(lib.pmce_embed_ln_f32(P(_c(pose2d)), P(_c(E)), P(_c(Wje)), P(_c(bje)), P(_c(spos)), P(x), BT * J, J, Cc, P(_c(w2)), P(_c(b2)), eps2,
                                     P(xn), int(xn_split), _st()), "embed_ln")
    return x, xn


def lifter_head(x, lnw, lnb, Wr, br, wf, bf, B, T, J, pre=None):
    """Regression head + frame fusion (PoseEstimation.py:62-66,109-113): x [B*T*J, C] -> pose3d [B, J, 3].  pre = (weight, bias, eps): the rows
    pass through that LayerNorm first (the last block's norm_t folded into the head)."""
    lib = _lib.load()
    Cc = x.shape[1]
    out = torch.empty(B, J, 3, device=x.device, dtype=torch.float32)
    pw, pb, pe = (_c(pre[0]), _c(pre[1]), float(pre[2])) if pre is not None else (None, None, 0.0)
    _lib.check(lib.pmce_lifter_head_f32(P(_c(x)), P(pw), P(pb), pe, P(_c(lnw)), P(_c(lnb)), P(_c(Wr)), P(_c(br)), P(_c(wf)), P(_c(bf)), P(out),
                                        B, T, J, Cc, _st()), "lifter_head")
    return out


def _attention_out(qkv, Cc, out):
    """The [rows, C] fp32 result buffer of an attention call: a fresh one, or the caller's `out` (the rows no sequence of the call owns keep
    what they held)."""
    if out is None:
        return torch.empty(qkv.shape[0], Cc, device=qkv.device, dtype=torch.float32)
    if out.dtype != torch.float32 or tuple(out.shape) != (qkv.shape[0], Cc) or out.device != qkv.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float32 [{qkv.shape[0]}, {Cc}] tensor on {qkv.device}, "
                         f"got {out.dtype} {tuple(out.shape)} on {out.device}")
    return out


def seq_attention(qkv, nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, out_split=False, out=None):
    lib = _lib.load()
    qkv = _c(qkv)
    out = _attention_out(qkv, Cc, out)
    _lib.check(lib.pmce_seq_attention_f32(P(qkv), P(out), nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride,
                                          int(out_split), _st()), "seq_attention")
    return out


def seq_attention_split(qkv, nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, out=None):
    """The matrix-pipe attention of the split-f16 mode: fp32 q, k, v in, pre-split result out (see :func:`unsplit_rows_f16`)."""
    lib = _lib.load()
    qkv = _c(qkv)
    out = _attention_out(qkv, Cc, out)
    _lib.check(lib.pmce_seq_attention_split_f16(P(qkv), P(out), nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, _st()),
               "seq_attention_split_f16")
    return out


def lifter_attention(qkv, nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, out_split=False, out=None):
    """:func:`seq_attention` at every width the model accepts (C = 128, 256, 384, 512): the entry the model calls."""
    lib = _lib.load()
    qkv = _c(qkv)
    out = _attention_out(qkv, Cc, out)
    _lib.check(lib.pmce_lifter_attention_f32(P(qkv), P(out), nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride,
                                             int(out_split), _st()), "lifter_attention")
    return out


def lifter_attention_split(qkv, nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, out=None, out_form=None):
    """:func:`seq_attention_split` at every width the model accepts (C = 128, 256, 384, 512): the entry the model calls.  out_form (None:
    the entry without a form argument): 1 pre-split planes, 2 plain f16 rows (:func:`f16_rows`)."""
    lib = _lib.load()
    qkv = _c(qkv)
    out = _attention_out(qkv, Cc, out)
    if out_form is None:
        _lib.check(lib.pmce_lifter_attention_split_f16(P(qkv), P(out), nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, _st()),
                   "lifter_attention_split_f16")
    else:
        _lib.check(lib.pmce_lifter_attention_split_f16_form(P(qkv), P(out), nseq, N, Cc, seq_div, seq_lo, seq_hi, tok_stride, int(out_form),
                                                            _st()), "lifter_attention_split_f16_form")
    return out


def qkv_attention_fused(xn_planes, Wblk, wscale, bias, B, J, overflow_word=None):
    """Temporal block at C = 512: pre-split XN [B*16*J, 512] -> pre-split attention output, one kernel (qkv_attention_fused.hip).
    overflow_word: optional int32 device tensor of one element, set to 1 when a result is not finite."""
    lib = _lib.load()
    Cc = xn_planes.shape[1]
    out = torch.empty_like(xn_planes)
    _lib.check(lib.pmce_qkv_attention_fused_split_f16(P(xn_planes), P(Wblk), P(wscale), P(bias), P(out), B, J, Cc, P(overflow_word), _st()),
               "qkv_attention_fused_split_f16")
    return out


def unsplit_rows_f16(Ap):
    """The fp32 values a packed (hi | lo*2^11) f16 buffer stands for (float64, exact): inverse of :func:`split_rows_f16`."""
    M, K = Ap.shape
    h = Ap.contiguous().view(torch.float16).view(M, K // 16, 2, 16).double()
    return (h[:, :, 0] + h[:, :, 1] / 2048.0).reshape(M, K)


def vertex_init_gather(joints, vj_relation):
    lib = _lib.load()
    joints = _c(joints)
    B, J, _ = joints.shape
    vj = torch.as_tensor(np.asarray(vj_relation).astype(np.int32), device=joints.device)
    out = torch.empty(B, 431, 3, device=joints.device, dtype=torch.float32)
    _lib.check(lib.pmce_vertex_init_gather_f32(P(joints), P(vj), P(out), B, J, _st()), "vertex_init_gather")
    return out


def adaln_params(g, sd, names):
    """GB[B, len(names)*128]: [gamma(64)|beta(64)] per AdaLN instance, via the packed GEMM (CoevoDecoder.py:19-20,27-28)."""
    Wt = torch.cat([torch.cat([sd[n + ".mlp_gamma.weight"], sd[n + ".mlp_beta.weight"]], 0) for n in names], 0)
    bt = torch.cat([torch.cat([sd[n + ".mlp_gamma.bias"], sd[n + ".mlp_beta.bias"]], 0) for n in names], 0)
    return gemm_nt(g, _c(Wt), _c(bt))


# ---- the decoder's operators ---------------------------------------------------------------------------------------------------------------
# Every wrapper below takes, next to its operands, what a test needs to place a launch inside memory of its own making (nothing here is on the
# product path, which calls pmce_forward):
#   out= (and vt_out=, pose_out=, qkv=)  the caller's result tensor, written in place and returned, as seq_attention's `out`;
#   bufs=  a dict of the caller's scratch and intermediate buffers, each optional: "Kf" [B,64,64], "s0" [B,64], "Vf" [B,64,64], "img"
#          [B, pmce_ca_image_floats()], "scratch" [B,431,64] (the J > 23 form), "kv" [B,431,128], "jf" [B,J,64], "sab" (vertex_sab's scratch);
#   gb=    (GB, insts): a caller-made [B, W] view of the [gamma | beta] blocks - rows may be strided (gb_stride = the view's row stride), the
#          last dimension contiguous - and the instance index of each AdaLN of the wrapper, in the order its docstring names them;
#   coords= / embed=  the operands of the from-coordinates forms (the token features are then None).
def _vp(t):
    """Device pointer of a tensor that need not be contiguous (a strided GB view), or None."""
    return None if t is None else C.c_void_p(t.data_ptr())


def _gb_of(gb, g, sd, names):
    """-> (GB view, gb_stride, instance indices) of a wrapper's AdaLN instances `names`: the dense GB of adaln_params, or the caller's."""
    if gb is None:
        GB = adaln_params(g, sd, names)
        return GB, GB.shape[1], list(range(len(names)))
    GB, insts = gb
    if not (GB.is_cuda and GB.dtype == torch.float32 and GB.dim() == 2 and GB.stride(1) == 1) or len(insts) != len(names):
        raise ValueError(f"gb must be (an fp32 device view [B, W] with a contiguous last dimension, {len(names)} instance indices)")
    return GB, (GB.stride(0) if GB.shape[0] > 1 else GB.shape[1]), [int(i) for i in insts]


def _buf(t, shape, like, what):
    """A fresh fp32 buffer of `shape`, or the caller's (checked: a wrong size would let a kernel write past it)."""
    if t is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != like.device or not t.is_contiguous():
        raise ValueError(f"{what} must be a contiguous float32 {tuple(shape)} tensor on {like.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t


def _ca_w(sd, p):
    return {k: _c(sd[f"{p}.attn.{k}"]) for k in ("wq.weight", "wq.bias", "wk.weight", "wk.bias", "wv.weight", "wv.bias",
                                                 "proj.weight", "proj.bias")}


def ca_image_floats(J=None):
    """Floats per clip of ca_fold's f16 image: the row stride (J = None), or what a clip's row holds at J joints (the rest of the row is
    never written)."""
    lib = _lib.load()
    return lib.pmce_ca_image_floats() if J is None else lib.pmce_ca_image_floats_written(int(J))


def ca_fold(xk, xv, GB, gb_stride, insts, w, B, J, Kf=None, s0=None, Vf=None, img=None, embed=None, jf=None):
    """pmce_ca_fold_f32 on its own, on the caller's buffers (each of Kf / s0 / Vf / img may be None = not wanted): the vertex<-joint
    cross-attention's key / value side of a clip, folded.  insts = the instances of (normq, normk, normv) in GB; w = the attention's
    weights (`_ca_w`).  embed = (jt [B,J,3], joint_proj.weight, .bias, joint_pos_embed [J,64], proj_j2v_dim.weight, .bias, j2v_K_embed
    [J,64]) with xk = xv = None: pmce_joint_prep_f32 (jf [B,J,64] or None receives the joint features)."""
    lib = _lib.load()
    tail = (_vp(GB), gb_stride, insts[0], insts[1], insts[2], P(w["wq.weight"]), P(w["wq.bias"]), P(w["wk.weight"]), P(w["wk.bias"]),
            P(w["wv.weight"]), P(w["wv.bias"]), P(w["proj.weight"]), P(Kf), P(s0), P(Vf), P(img), B, J, _st())
    if embed is None:
        _lib.check(lib.pmce_ca_fold_f32(P(xk), P(xv), *tail), "ca_fold")
    else:
        _lib.check(lib.pmce_joint_prep_f32(*[P(e) for e in embed], P(jf), *tail), "joint_prep")


def _fold(xk, xv, g, sd, p, names, gb, bufs, B, J, embed, want_img, like):
    """The fold of a composite wrapper: -> (GB, gb_stride, insts, w, Kf, s0, Vf, img)."""
    bufs = bufs or {}
    GB, gbs, insts = _gb_of(gb, g, sd, names)
    w = _ca_w(sd, p)
    Kf = _buf(bufs.get("Kf"), (B, 64, 64), like, "Kf")
    s0 = _buf(bufs.get("s0"), (B, 64), like, "s0")
    Vf = _buf(bufs.get("Vf"), (B, 64, 64), like, "Vf")
    img = _buf(bufs.get("img"), (B, ca_image_floats()), like, "img") if want_img else None
    jf = bufs.get("jf")
    if embed is not None:
        embed = [_c(e) for e in embed]
        if jf is not None:
            jf = _buf(jf, (B, J, 64), like, "jf")
    ca_fold(xk, xv, GB, gbs, insts, w, B, J, Kf, s0, Vf, img, embed, jf)
    return GB, gbs, insts, w, Kf, s0, Vf, img


def _query_side(xq, coords):
    """-> (xq or None, vt, Wv3, Eq, B, a tensor on the device): explicit query tokens, or coords = (vt [B,431,3], vertx_proj.weight [64,3],
    Eq [431,64] = vertx_proj.bias + vertx_pos_embed + v_Q_embed)."""
    if coords is None:
        xq = _c(xq)
        assert xq.shape[1] == 431
        return xq, None, None, None, xq.shape[0], xq
    vt, Wv3, Eq = (_c(t) for t in coords)
    assert xq is None and vt.shape[1] == 431
    return None, vt, Wv3, Eq, vt.shape[0], vt


def cross_attn_vertex(xq, xk, xv, g, sd, p, out=None, gb=None, bufs=None, coords=None, embed=None):
    """Fused AdaLN + vertex<-joint cross-attention + residual: xq + CA(AdaLN_q(xq), AdaLN_k(xk), AdaLN_v(xv))
    (first line of CrossAttentionBlock.forward, CoevoDecoder.py:83) with p = '...vertx_CA_FFN'.  AdaLN order of gb: normq, normk, normv.
    coords: the query tokens from the vertex coordinates (`_query_side`); embed: the key side from the joints (`ca_fold`)."""
    lib = _lib.load()
    xq, vt, Wv3, Eq, B, like = _query_side(xq, coords)
    if embed is None:
        xk, xv = _c(xk), _c(xv)
    J = xk.shape[1] if embed is None else embed[0].shape[1]
    _, _, _, w, Kf, s0, Vf, _ = _fold(xk, xv, g, sd, p, [p + ".normq", p + ".normk", p + ".normv"], gb, bufs, B, J, embed, False, like)
    out = _buf(out, (B, 431, 64), like, "out")
    _lib.check(lib.pmce_vertex_ca_f32(P(xq), P(vt), P(Wv3), P(Eq), P(Kf), P(s0), P(Vf), P(w["proj.bias"]), P(out), B, J, _st()),
               "vertex_ca")
    return out


def ffn_image(fc1_w, fc2_w):
    """The LDS image of a 64->256->64 FFN's f16 form (pmce_ffn_pack_f16): what pmce_model_finalize makes per decoder FFN."""
    lib = _lib.load()
    fc1_w, fc2_w = _c(fc1_w), _c(fc2_w)
    assert tuple(fc1_w.shape) == (256, 64) and tuple(fc2_w.shape) == (64, 256)
    img = torch.empty(lib.pmce_ffn_image_floats(), device=fc1_w.device)
    _lib.check(lib.pmce_ffn_pack_f16(P(fc1_w), P(fc2_w), P(img), _st()), "ffn_pack_f16")
    return img


def cross_attn_block_vertex(xq, xk, xv, g, sd, p, split_f16=False, packed=False, out=None, gb=None, bufs=None, coords=None, embed=None):
    """The whole vertex-stream CrossAttentionBlock in one launch (CoevoDecoder.py:82-87), p = '...vertx_CA_FFN':
    xq + CA(...) then + Mlp(AdaLN_2(.)).  fp32 form: bit-identical to cross_attn_vertex followed by adaln_mlp.  split_f16: the FFN and
    (round 5, J <= 23) the attention's two contractions in the three-product f16 form - the folded key / value operands reach the kernel as
    the f16 image ca_fold writes.  packed (with split_f16): the FFN's planes from a pre-made image (ffn_image) instead of converted per
    workgroup.  AdaLN order of gb: normq, normk, normv, norm2.  coords / embed: see cross_attn_vertex."""
    lib = _lib.load()
    xq, vt, Wv3, Eq, B, like = _query_side(xq, coords)
    if embed is None:
        xk, xv = _c(xk), _c(xv)
    J = xk.shape[1] if embed is None else embed[0].shape[1]
    names = [p + ".normq", p + ".normk", p + ".normv", p + ".norm2"]
    GB, gbs, insts, w, Kf, s0, Vf, img = _fold(xk, xv, g, sd, p, names, gb, bufs, B, J, embed, split_f16 and J <= 23, like)
    m = [_c(sd[p + k]) for k in (".mlp.fc1.weight", ".mlp.fc1.bias", ".mlp.fc2.weight", ".mlp.fc2.bias")]
    out = _buf(out, (B, 431, 64), like, "out")
    scratch = _buf((bufs or {}).get("scratch"), (B, 431, 64), like, "scratch") if J > 23 else None
    fimg = ffn_image(m[0], m[2]) if packed else None
    _lib.check(lib.pmce_vertex_ca_mlp_f32(P(xq), P(vt), P(Wv3), P(Eq), P(Kf), P(s0), P(Vf), P(w["proj.bias"]), _vp(GB), gbs,
                                          insts[3], P(m[0]), P(m[1]), P(m[2]), P(m[3]), P(out), P(scratch), B, J,
                                          1 if split_f16 else 0, P(fimg), P(img), _st()), "vertex_ca_mlp")
    return out


def adaln_mlp(x, g, sd, p_norm, p_mlp, coor=None, vt_in=None, want_features=True, split_f16=False, packed=False, out=None, vt_out=None,
              gb=None):
    """x + Mlp(AdaLN(x)) on [B,431,64]; optional coordinate head (Wc[3,64], bc[3]) + vt_in residual.  packed: see cross_attn_block_vertex."""
    lib = _lib.load()
    x = _c(x)
    B = x.shape[0]
    GB, gbs, insts = _gb_of(gb, g, sd, [p_norm])
    w = [_c(sd[p_mlp + k]) for k in (".fc1.weight", ".fc1.bias", ".fc2.weight", ".fc2.bias")]
    y = _buf(out, tuple(x.shape), x, "out") if want_features else None
    Wc = bc = None
    if coor is None and vt_out is not None:
        raise ValueError("adaln_mlp: vt_out needs the coordinate head (coor, vt_in)")
    if coor is not None:
        Wc, bc = _c(coor[0]), _c(coor[1])
        vt_in = _c(vt_in)
        vt_out = _buf(vt_out, tuple(vt_in.shape), x, "vt_out")
    img = ffn_image(w[0], w[2]) if packed else None
    _lib.check(lib.pmce_adaln_mlp_f32(P(x), _vp(GB), gbs, insts[0], P(w[0]), P(w[1]), P(w[2]), P(w[3]), P(y), P(Wc), P(bc),
                                      P(vt_in), P(vt_out), B, 1 if split_f16 else 0, P(img), _st()), "adaln_mlp")
    return y, vt_out


def vertex_self_attn(x, g, sd, p, split_f16=False, out=None, qkv=None, gb=None, bufs=None):
    """x + SA(AdaLN(x)) on [B,431,64], 2 heads (first line of Block.forward, CoevoDecoder.py:103); p = '...vertx_SA_FFN'.
    fp32 pipe: two launches (adaln_qkv, vertex_sa), returns (y, qkv).  split_f16: ONE launch (pmce_vertex_sab_split_f32: AdaLN + qkv
    product + attention + proj + residual, every contraction but the projection as three f16 matrix products; what a model in split_f16
    mode runs), returns (y, None) - no fp32 qkv exists."""
    lib = _lib.load()
    x = _c(x)
    B = x.shape[0]
    GB, gbs, insts = _gb_of(gb, g, sd, [p + ".norm1"])
    Wqkv = _c(sd[p + ".attn.qkv.weight"])
    y = _buf(out, tuple(x.shape), x, "out")
    if split_f16:
        img = torch.empty(lib.pmce_qkv_image_floats(), device=x.device)
        _lib.check(lib.pmce_qkv_pack_f16(P(Wqkv), P(img), _st()), "qkv_pack_f16")
        scratch = _buf((bufs or {}).get("sab"), (lib.pmce_vertex_sab_scratch_floats(B),), x, "sab")
        _lib.check(lib.pmce_vertex_sab_split_f32(P(x), _vp(GB), gbs, insts[0], P(img), P(_c(sd[p + ".attn.qkv.bias"])),
                                                 P(_c(sd[p + ".attn.proj.weight"])), P(_c(sd[p + ".attn.proj.bias"])), P(scratch), P(y), B,
                                                 _st()), "vertex_sab")
        return y, None
    qkv = _buf(qkv, (B, 431, 192), x, "qkv")
    _lib.check(lib.pmce_adaln_qkv_f32(P(x), _vp(GB), gbs, insts[0], P(Wqkv), P(_c(sd[p + ".attn.qkv.bias"])), P(qkv), B, _st()), "adaln_qkv")
    _lib.check(lib.pmce_vertex_sa_f32(P(x), P(qkv), P(_c(sd[p + ".attn.proj.weight"])), P(_c(sd[p + ".attn.proj.bias"])), P(y), B, _st()),
               "vertex_sa")
    return y, qkv


def tokens_kv(xk, xv, g, sd, ca, split_f16=False, kv=None, gb=None, coords=None):
    """pmce_tokens_kv_f32 on its own: kv [B,431,128] = Wk AdaLN_k(xk) + bk | Wv AdaLN_v(xv) + bv of the joint<-vertex cross-attention
    (ca = '...joint_CA_FFN').  AdaLN order of gb: normk, normv.  coords = (vt [B,431,3], vertx_proj.weight [64,3], Ev [431,64] =
    vertx_proj.bias + vertx_pos_embed, proj_v2j_dim.weight [64,64], Ek [431,64] = proj_v2j_dim.bias + v2j_K_embed) with xk = xv = None:
    xv = Wv3 vt + Ev, xk = Wv2j xv + Ek formed in the kernel.  split_f16: the 64 x 64 products in the three-product f16 form from the
    weights' image, proj_v2j_dim.weight in its first slot when coords are given."""
    lib = _lib.load()
    vt = Wv3 = Ev = Wv2j = Ek = None
    if coords is None:
        xk, xv = _c(xk), _c(xv)
        B, like = xk.shape[0], xk
    else:
        assert xk is None and xv is None
        vt, Wv3, Ev, Wv2j, Ek = (_c(t) for t in coords)
        B, like = vt.shape[0], vt
    GB, gbs, insts = _gb_of(gb, g, sd, [ca + ".normk", ca + ".normv"])
    kv = _buf(kv, (B, 431, 128), like, "kv")
    Wk, Wv = _c(sd[ca + ".attn.wk.weight"]), _c(sd[ca + ".attn.wv.weight"])
    img = None
    if split_f16:   # (the generic form does not use proj_v2j_dim: any 64 x 64 weight fills the image's first slot)
        img = torch.empty(lib.pmce_tkv_image_floats(), device=like.device)
        _lib.check(lib.pmce_tkv_pack_f16(P(Wk if Wv2j is None else Wv2j), P(Wk), P(Wv), P(img), _st()), "tkv_pack_f16")
    _lib.check(lib.pmce_tokens_kv_f32(P(xk), P(xv), P(vt), P(Wv3), P(Ev), P(Wv2j), P(Ek), _vp(GB), gbs, insts[0], insts[1],
                                      P(Wk), P(_c(sd[ca + ".attn.wk.bias"])), P(Wv), P(_c(sd[ca + ".attn.wv.bias"])), P(kv), B,
                                      P(img), _st()), "tokens_kv")
    return kv


def joint_stream(xq, xk, xv, g, sd, blk, stage, jt=None, split_f16=False, out=None, pose_out=None, gb=None, bufs=None, coords=None,
                 jQ=None):
    """Joint stream of a CoevoBlock given explicit q/k/v token sets (xq[B,J,64], xk/xv[B,431,64]):
    stage 1 = xq + CA (CoevoDecoder.py:83), 2 = + FFN (:85-86), 3 = + joint_SA_FFN (:187) (+ coords if jt).
    split_f16: the k / v products over the 431 vertex tokens (tokens_kv) in the three-product f16 form from the weights' image.
    AdaLN order of gb: joint_CA_FFN's normq, normk, normv, norm2, joint_SA_FFN's norm1, norm2.  coords: see tokens_kv; jQ [J,64]: added
    to xq in the kernel (j_Q_embed)."""
    lib = _lib.load()
    xq = _c(xq)
    B, J, _ = xq.shape
    ca, sa = blk + ".joint_CA_FFN", blk + ".joint_SA_FFN"
    GB, gbs, insts = _gb_of(gb, g, sd, [ca + ".normq", ca + ".normk", ca + ".normv", ca + ".norm2", sa + ".norm1", sa + ".norm2"])
    kv = tokens_kv(xk, xv, g, sd, ca, split_f16, (bufs or {}).get("kv"), (GB, insts[1:3]), coords)
    names = [ca + ".attn.wq.weight", ca + ".attn.wq.bias", ca + ".attn.proj.weight", ca + ".attn.proj.bias",
             ca + ".mlp.fc1.weight", ca + ".mlp.fc1.bias", ca + ".mlp.fc2.weight", ca + ".mlp.fc2.bias",
             sa + ".attn.qkv.weight", sa + ".attn.qkv.bias", sa + ".attn.proj.weight", sa + ".attn.proj.bias",
             sa + ".mlp.fc1.weight", sa + ".mlp.fc1.bias", sa + ".mlp.fc2.weight", sa + ".mlp.fc2.bias",
             blk + ".proj_joint_feat2coor.weight", blk + ".proj_joint_feat2coor.bias"]
    ws = [_c(sd[n]) for n in names]
    wptr = (C.c_void_p * 18)(*[w.data_ptr() for w in ws])
    inst = (C.c_int * 4)(insts[0], insts[3], insts[4], insts[5])
    y = _buf(out, (B, J, 64), xq, "out")
    pose = None
    if jt is not None:
        jt = _c(jt)
        pose = _buf(pose_out, (B, J, 3), xq, "pose_out")
    _lib.check(lib.pmce_joint_stream_f32(P(xq), P(None if jQ is None else _c(jQ)), P(kv), _vp(GB), gbs, wptr, inst, P(jt), P(y), P(pose),
                                         B, J, stage, _st()), "joint_stream")
    return y, pose, kv


def joint_self_attn_block(x, g, sd, blk, out=None, gb=None):
    """joint_SA_FFN alone: x + SA(AdaLN(x)); x + Mlp(AdaLN(x)) on [B,J,64], 8 heads (the reference's Block module,
    CoevoDecoder.py:102-105) - joint_stream's stage 4.  AdaLN order of gb: norm1, norm2."""
    lib = _lib.load()
    x = _c(x)
    B, J, _ = x.shape
    sa = blk + ".joint_SA_FFN"
    GB, gbs, insts = _gb_of(gb, g, sd, [sa + ".norm1", sa + ".norm2"])
    names = [sa + ".attn.qkv.weight"] * 8 + [sa + ".attn.qkv.weight", sa + ".attn.qkv.bias", sa + ".attn.proj.weight",
                                             sa + ".attn.proj.bias", sa + ".mlp.fc1.weight", sa + ".mlp.fc1.bias",
                                             sa + ".mlp.fc2.weight", sa + ".mlp.fc2.bias"] + [sa + ".attn.qkv.weight"] * 2
    ws = [_c(sd[n]) for n in names]            # slots 0-7 (cross-attention block) and 16-17 (coordinate head) are unused
    wptr = (C.c_void_p * 18)(*[w.data_ptr() for w in ws])
    inst = (C.c_int * 4)(insts[0], insts[0], insts[0], insts[1])
    y = _buf(out, (B, J, 64), x, "out")
    _lib.check(lib.pmce_joint_stream_f32(P(x), None, None, _vp(GB), gbs, wptr, inst, None, P(y), None, B, J, 4, _st()),
               "joint_stream(stage 4)")
    return y


def coevo_block(model, k, joints, vt_in, g):
    """CoevoBlock k of a pmce_amd.models.{PMCE,CoevoDecoder} instance on explicit inputs (CoevoDecoder.py:175-191):
    -> (vt_out[B,431,3], joint_out[B,J,3] or None for k < 3)."""
    eng = model._ensure_packed()
    joints, vt_in, g = _c(joints), _c(vt_in), _c(g)
    B = joints.shape[0]
    vt_out = torch.empty_like(vt_in)
    j_out = torch.empty_like(joints) if k == 3 else None
    ws = eng.workspace(B)
    _lib.check(eng.lib.pmce_coevo_block_forward(eng.handle, k, P(joints), P(vt_in), P(g), P(vt_out), P(j_out), B,
                                                C.c_void_p(ws.data_ptr()), ws.numel(), _st()), "coevo_block_forward")
    return vt_out, j_out


def final_product(model, vt, g):
    """cam_mesh[B,6890,3] = upsample_conv(vt) + cat(linear_cur1..3(relu(g)))  (CoevoDecoder.py:238-244) through the packed
    [20670, 3360] operand of a pmce_amd model."""
    lib = _lib.load()
    eng = model._ensure_packed()
    vt, g = _c(vt), _c(g)
    B = vt.shape[0]
    KP = eng.packed["dec.final.weight"].shape[1]
    A = torch.empty(B, KP, device=vt.device, dtype=torch.float32)
    _lib.check(lib.pmce_build_final_operand_f32(P(g), P(vt), P(A), B, KP, 0, _st()), "build_final_operand")
    return gemm_nt(A, eng.packed["dec.final.weight"], eng.packed["dec.final.bias"]).reshape(B, 6890, 3)


def j_regress(cam_mesh_m, j_regressor, scale=1000.0):
    """J_regressor[None] @ (cam_mesh*1000) (lib/core/base.py:223-225); j_regressor dense [R,6890] (numpy or tensor)."""
    from .assets import regressor_to_csr
    lib = _lib.load()
    mesh = _c(cam_mesh_m)
    B = mesh.shape[0]
    jr = j_regressor.detach().cpu().numpy() if isinstance(j_regressor, torch.Tensor) else np.asarray(j_regressor)
    indptr, indices, data = regressor_to_csr(jr)
    dev = mesh.device
    ip, ix, dt = (torch.from_numpy(a).to(dev) for a in (indptr, indices, data))
    out = torch.empty(B, jr.shape[0], 3, device=dev, dtype=torch.float32)
    _lib.check(lib.pmce_j_regress_f32(P(mesh), P(ip), P(ix), P(dt), P(out), B, jr.shape[0], mesh.shape[1], scale, _st()),
               "j_regress")
    return out


def render_workspace_bytes(n_jobs, n_verts, width, height, chunk_frames=1):
    """Bytes of workspace pmce_render_meshes needs to process ``chunk_frames`` frames per chunk (1 = the least it accepts)."""
    b = int(_lib.load().pmce_render_workspace_bytes(int(n_jobs), int(n_verts), int(width), int(height), int(chunk_frames)))
    if b == 0:
        raise _lib.PmceError(f"render_workspace_bytes: {_lib.last_error()}")
    return b


def render_meshes(images, verts, cams, rotation, faces, vf_offsets, vf_faces, job_frame_host, job_frame, sched_host, sched,
                  layer_offsets_host, material, lights, cull_backfaces, depth_order, status, xy_fixed, face_id, depth, workspace):
    """pmce_render_meshes on the current stream, in place on images uint8 [F,H,W,3] (pmce_amd.render.Renderer prepares the tables: faces,
    the vertex -> face CSR and the job tables on the device, the schedule int32 numpy arrays on the host, material float32[6] and
    lights float32[K,3] on the host).  rotation, xy_fixed, face_id and depth may be None."""
    lib = _lib.load()
    F, H, W, _ = images.shape
    N, V, _ = verts.shape
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))      # noqa: E731
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))    # noqa: E731
    for a in (job_frame_host, sched_host, layer_offsets_host):
        assert a.dtype == np.int32 and a.flags.c_contiguous
    assert material.dtype == np.float32 and lights.dtype == np.float32 and images.dtype == torch.uint8
    _lib.check(lib.pmce_render_meshes(P(images), F, W, H, P(verts), P(cams), P(rotation), N, V, P(faces), faces.shape[0], P(vf_offsets),
                                      P(vf_faces), ip(job_frame_host), P(job_frame), ip(sched_host), P(sched), ip(layer_offsets_host),
                                      len(layer_offsets_host) - 1, fp(material), fp(lights), len(lights), 1 if cull_backfaces else 0,
                                      1 if depth_order else 0, P(status), P(xy_fixed), P(face_id), P(depth),
                                      C.c_void_p(workspace.data_ptr()), workspace.numel(), _st()), "render_meshes")
    return images


def smpl_workspace_bytes(B):
    """Bytes of workspace pmce_smpl_forward needs for a batch of B rows."""
    b = int(_lib.load().pmce_smpl_workspace_bytes(int(B)))
    if b == 0:
        raise _lib.PmceError(f"smpl_workspace_bytes: {_lib.last_error()}")
    return b


def smpl_forward(model, pose, betas, trans, cam_R, cam_t, sample_index, scale, offset, verts_out, joints_out, workspace):
    """pmce_smpl_forward on the current stream, in place on verts_out [B,V,3] and joints_out [B,24,3] (pmce_amd.smpl.SMPL prepares the
    arguments: `model` a smpl.SMPLModel, sample_index an int32 device tensor of the rows to compute or None for all; trans, cam_R + cam_t
    and offset may be None)."""
    lib = _lib.load()
    B, V = verts_out.shape[0], verts_out.shape[1]
    vt, dirs, wts, jt, jsd = model.to(verts_out.device)
    if vt.shape[1] != V:
        raise _lib.PmceError(f"smpl_forward: the model has {vt.shape[1]} vertices, verts_out {V}")
    par = np.ascontiguousarray(model.parents, dtype=np.int32)
    if sample_index is not None:
        assert sample_index.dtype == torch.int32
    n = B if sample_index is None else int(sample_index.numel())
    _lib.check(lib.pmce_smpl_forward(P(vt), P(dirs), P(wts), P(jt), P(jsd), par.ctypes.data_as(C.POINTER(C.c_int)), len(par), P(pose),
                                     P(betas), P(trans), P(cam_R), P(cam_t), P(sample_index), n, scale, P(offset), P(verts_out),
                                     P(joints_out), C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size(), B, V,
                                     _st()), "smpl_forward")
    return verts_out, joints_out


def smpl_forward_rotmat(model, rotmats, betas, trans, sample_index, scale, offset, verts_out, joints_out, workspace):
    """pmce_smpl_forward_rotmat on the current stream, in place on verts_out [B,V,3] and joints_out [B,24,3]: rotmats [B,24,3,3]
    contiguous, betas [B,10] with unit column stride and any row stride >= 10 (read in place); the rest as for smpl_forward."""
    lib = _lib.load()
    B, V = verts_out.shape[0], verts_out.shape[1]
    vt, dirs, wts, jt, jsd = model.to(verts_out.device)
    if vt.shape[1] != V:
        raise _lib.PmceError(f"smpl_forward_rotmat: the model has {vt.shape[1]} vertices, verts_out {V}")
    par = np.ascontiguousarray(model.parents, dtype=np.int32)
    assert betas.stride(1) == 1 and betas.is_cuda and betas.dtype == torch.float32
    if sample_index is not None:
        assert sample_index.dtype == torch.int32
    n = B if sample_index is None else int(sample_index.numel())
    _lib.check(lib.pmce_smpl_forward_rotmat(P(vt), P(dirs), P(wts), P(jt), P(jsd), par.ctypes.data_as(C.POINTER(C.c_int)), len(par),
                                            P(rotmats), C.c_void_p(betas.data_ptr()), int(betas.stride(0)) if B > 1 else 10, P(trans),
                                            P(sample_index), n, scale, P(offset), P(verts_out), P(joints_out),
                                            C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size(), B, V, _st()),
               "smpl_forward_rotmat")
    return verts_out, joints_out


def smpl_fit_workspace_bytes(B, V):
    """Bytes of workspace pmce_smpl_fit needs for B meshes of V vertices; raises where V is more than a workgroup's LDS holds."""
    b = int(_lib.load().pmce_smpl_fit_workspace_bytes(int(B), int(V)))
    if b == 0:
        raise _lib.PmceError(f"smpl_fit_workspace_bytes: {_lib.last_error()}")
    return b


def smpl_fit(model, verts, init_rotmats, init_betas, init_trans, sample_index, n_sweeps, fit_shape, rotmats, pose, betas, trans, residual,
             status, history, workspace):
    """pmce_smpl_fit on the current stream, in place on rotmats [B,24,3,3], pose [B,72], betas [B,10], trans [B,3], residual [B], status
    [B] int32 and history [B,n_sweeps] or None (pmce_amd.smpl.SMPL.fit prepares the arguments: `model` a smpl.SMPLModel, verts [B,V,3]
    contiguous fp32, the three init tensors contiguous or None, sample_index an int32 device tensor of the rows to fit or None)."""
    lib = _lib.load()
    B, V = verts.shape[0], verts.shape[1]
    vt, dirs, wts, jt, jsd = model.to(verts.device)
    sub = model.subtree_to(verts.device)
    if vt.shape[1] != V:
        raise _lib.PmceError(f"smpl_fit: the model has {vt.shape[1]} vertices, verts {V}")
    par = np.ascontiguousarray(model.parents, dtype=np.int32)
    assert verts.dtype == torch.float32 and verts.is_contiguous() and status.dtype == torch.int32
    if sample_index is not None:
        assert sample_index.dtype == torch.int32
    n = B if sample_index is None else int(sample_index.numel())
    _lib.check(lib.pmce_smpl_fit(P(vt), P(dirs), P(wts), P(sub), P(jt), P(jsd), par.ctypes.data_as(C.POINTER(C.c_int)), len(par), P(verts),
                                 P(init_rotmats), P(init_betas), P(init_trans), P(sample_index), n, int(n_sweeps), 1 if fit_shape else 0,
                                 P(rotmats), P(pose), P(betas), P(trans), P(residual), P(status), P(history),
                                 C.c_void_p(workspace.data_ptr()), workspace.numel() * workspace.element_size(), B, V, _st()), "smpl_fit")


def hmr_head(features, q_t, cst, pmi_t, init, state, rotmat, theta):
    """pmce_hmr_head_f32 on the current stream: features [n,2048], q_t [2048,160], cst [157], pmi_t [157,160] = (P - I)^T + init [n,157] or
    None + None -> state [n,157], rotmat [n,24,3,3], theta [n,85], written in place."""
    n = features.shape[0]
    _lib.check(_lib.load().pmce_hmr_head_f32(P(features), P(q_t), P(cst), P(pmi_t), P(init), n, P(state), P(rotmat), P(theta), _st()),
               "hmr_head")
    return state, rotmat, theta


def hmr_joints(joints, verts, sel, indptr, indices, data, cam, cam_stride, kp_3d, kp_2d):
    """pmce_hmr_joints_f32 on the current stream: joints [n,24,3], verts [n,V,3], the joint table (sel int32 [K], CSR int32 / int32 / fp32)
    on the device, cam = a device tensor whose rows start with the camera at a stride of cam_stride floats -> kp_3d [n,K,3], kp_2d [n,K,2]."""
    n, V, K = verts.shape[0], verts.shape[1], sel.shape[0]
    _lib.check(_lib.load().pmce_hmr_joints_f32(P(joints), P(verts), P(sel), P(indptr), P(indices), P(data), C.c_void_p(cam.data_ptr()),
                                               int(cam_stride), n, K, V, P(kp_3d), P(kp_2d), _st()), "hmr_joints")
    return kp_3d, kp_2d


def overlay_workspace_bytes(width, height, chunk_frames=1):
    """Bytes of workspace pmce_draw_overlays needs to process ``chunk_frames`` frames per chunk (1 = the least it accepts)."""
    b = int(_lib.load().pmce_overlay_workspace_bytes(int(width), int(height), int(chunk_frames)))
    if b == 0:
        raise _lib.PmceError(f"overlay_workspace_bytes: {_lib.last_error()}")
    return b


def draw_overlays(frames, frame_index_host, frame_index, boxes, box_format, ids, keypoints, skeleton, score_thresh, thickness, radius, label_scale, font,
                  palette, text_color, alpha, status, workspace):
    """pmce_draw_overlays on the current stream, in place on frames uint8 [F,H,W,3] (pmce_amd.overlay.draw prepares the tables):
    frame_index int32 [N] (frame_index_host: the same table as an int32 numpy array when it is ascending, else None), boxes fp64 [N,4], ids int64 [N], keypoints fp64 [N,K,2 or 3], skeleton int32 [L,2], font uint8 [10,7] and
    palette uint8 [P,3] on the device, text_color uint8 [3] on the host; box_format the C entry's code.  boxes, ids and keypoints may
    be None."""
    lib = _lib.load()
    F, H, W, _ = frames.shape
    assert frames.dtype == torch.uint8 and frame_index.dtype == torch.int32 and status.dtype == torch.int32
    assert boxes is None or boxes.dtype == torch.float64
    assert ids is None or ids.dtype == torch.int64
    assert keypoints is None or keypoints.dtype == torch.float64
    assert skeleton.dtype == torch.int32 and font.dtype == torch.uint8 and palette.dtype == torch.uint8
    assert frame_index_host is None or (frame_index_host.dtype == np.int32 and frame_index_host.flags.c_contiguous and
                                        frame_index_host.shape == tuple(frame_index.shape))
    assert text_color.dtype == np.uint8 and text_color.shape == (3,) and text_color.flags.c_contiguous
    K, D = (keypoints.shape[1], keypoints.shape[2]) if keypoints is not None else (0, 0)
    _lib.check(lib.pmce_draw_overlays(P(frames), F, W, H,
                                      None if frame_index_host is None else frame_index_host.ctypes.data_as(C.POINTER(C.c_int)),
                                      P(frame_index), P(boxes), int(box_format), P(ids), P(keypoints), K, D,
                                      P(skeleton) if skeleton.numel() else None, skeleton.shape[0], float(score_thresh), thickness, radius,
                                      label_scale, P(font), P(palette), palette.shape[0], text_color.ctypes.data_as(C.POINTER(C.c_ubyte)),
                                      alpha, frame_index.shape[0], P(status), C.c_void_p(workspace.data_ptr()), workspace.numel(), _st()),
               "draw_overlays")
    return frames
