"""CPU-only tests of the host side: the C-ABI library loads and exports every declared symbol, argument
validation works without a GPU, the façade modules keep the reference's checkpoint layout, and the load-time
weight packing is equivalent to the reference arithmetic it replaces."""
import os
import os.path as osp
import re

import numpy as np
import pytest
import torch

from conftest import REPO, cached_state_dict


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


def test_f16_matrix_kernels_contain_no_packed_fp32(lib, tmp_path):
    """No kernel of the library may contain packed-fp32 vector instructions: on MI355X those get disturbed by f16 matrix
    instructions of co-resident waves - of other kernels and of the same kernel.  Checked on the device code of
    EVERY object the library was linked from (the packed-fp32 bystander kernels of the interference report live in the separate
    diagnostics library, scripts/microbench/libpmce_diag.so)."""
    import shutil
    import subprocess
    from pmce_amd import build as B
    B.build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not osp.exists(objdump):
        pytest.skip("llvm-objdump not available")
    assert set(B.FILE_FLAGS) == {s for s in B.SOURCES if s.endswith(".hip")}
    f16_files = set()
    for src in B.FILE_FLAGS:
        obj = osp.join(B.CSRC, "build", osp.splitext(src)[0] + ".o")
        if not osp.exists(obj):
            pytest.skip(f"{obj} not present (library built elsewhere)")
        local = str(tmp_path / osp.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True)
        dev = [f for f in os.listdir(tmp_path) if f.startswith(osp.basename(obj) + ".") and "amdgcn" in f]
        assert dev, f"no device code object extracted from {obj}"
        asm = subprocess.run([objdump, "-d", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
        if "v_mfma_f32_32x32x16_f16" in asm or "v_mfma_f32_16x16x32_f16" in asm:
            f16_files.add(src)
        bad = sorted(set(re.findall(r"v_pk_(?:fma|mul|add)_f32", asm)))
        assert not bad, f"{src}: packed-fp32 instructions {bad} in a library whose kernels issue f16 matrix instructions"
    assert f16_files == {"gemm_split_f16.hip", "gemm_split_small.hip", "gemm_f16.hip", "seq_attention_mfma.hip", "vit_attention.hip", "conv.hip",
                         "gru.hip", "coevo.hip"}


def test_library_exports_every_declared_symbol(lib):
    import ctypes
    from pmce_amd import _lib
    hdr = open(osp.join(REPO, "include", "pmce_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pmce_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 30
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in sorted(declared):
        assert hasattr(raw, name), f"{name} declared in include/pmce_hip.h but not exported"
    assert declared == set(_lib.PROTOTYPES), declared ^ set(_lib.PROTOTYPES)
    assert lib.pmce_version() == 100
    # ... and the converse: every dynamic symbol the library defines whose unmangled name starts with pmce_ is declared in the header
    # (the internal helpers are C++-mangled and do not match)
    import subprocess
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not osp.exists(objdump):
        pytest.skip("llvm-objdump not available")
    table = subprocess.run([objdump, "-T", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {f[-1] for f in (l.split() for l in table.splitlines()) if len(f) >= 4 and "*UND*" not in f and f[-1].startswith("pmce_")}
    assert exported == declared, exported ^ declared


def test_argument_validation_without_gpu(lib):
    from pmce_amd import _lib
    rc = lib.pmce_gemm_nt_f32(1, 1, None, None, 1, 8, 8, 33, 33, 36, 8, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, None)
    assert rc == -1 and "K%32" in _lib.last_error()
    rc = lib.pmce_seq_attention_f32(1, 1, 4, 40, 256, 0, 1, 0, 1, 0, None)
    assert rc == -1 and "1..32" in _lib.last_error()
    assert lib.pmce_seq_attention_split_supported(17, 512) == 1 and lib.pmce_seq_attention_split_supported(16, 256) == 1
    assert lib.pmce_seq_attention_split_supported(24, 512) == 0 and lib.pmce_seq_attention_split_supported(17, 384) == 0
    rc = lib.pmce_seq_attention_split_f16(16, 16, 4, 24, 512, 0, 24, 0, 1, None)
    assert rc == -1 and "16, 17 or 19" in _lib.last_error()
    import ctypes as C
    h = C.c_void_p()
    assert lib.pmce_model_create(17, 300, 3, C.byref(h)) == -1
    assert lib.pmce_model_create(19, 512, 3, C.byref(h)) == 0
    names = [lib.pmce_model_tensor_name(h, i).decode() for i in range(lib.pmce_model_tensor_count(h))]
    assert "dec.final.weight" in names and "lifter.SpatialBlocks.2.mlp.fc2.bias" in names
    assert lib.pmce_model_set_tensor(h, b"nope", 16) == -1
    assert lib.pmce_model_finalize(h) == -1                      # nothing registered
    assert lib.pmce_model_workspace_bytes(h, 64) > 0
    assert lib.pmce_forward(h, 16, 16, 16, 16, 16, None, 1, 256, 1 << 40, None) == -1   # not finalized
    lib.pmce_model_destroy(h)


def test_the_five_environment_knobs(lib, monkeypatch):
    """the library reads exactly five environment variables, all in pmce_model_create, each the initial value of a
    setting with an API setter and getter (include/pmce_hip.h at pmce_model_create).  Every one is flipped here (creating a handle needs
    no GPU), and no other PMCE_* name is read anywhere in the library's sources."""
    import ctypes as C

    def create():
        h = C.c_void_p()
        assert lib.pmce_model_create(17, 256, 3, C.byref(h)) == 0
        st = dict(split=lib.pmce_model_gemm_mode(h), min_batch=lib.pmce_model_get_split_min_batch(h), strict=lib.pmce_model_get_overflow_policy(h),
                  two_streams=lib.pmce_model_get_concurrency(h), overlap=lib.pmce_model_get_split_overlap(h))
        lib.pmce_model_destroy(h)
        return st

    for k in ("PMCE_SPLIT_F16", "PMCE_SPLIT_MIN_BATCH", "PMCE_STRICT_OVERFLOW", "PMCE_SINGLE_STREAM", "PMCE_SPLIT_OVERLAP"):
        monkeypatch.delenv(k, raising=False)
    base = create()
    assert base == dict(split=1, min_batch=1, strict=0, two_streams=1, overlap=1)
    for var, val, key, want in (("PMCE_SPLIT_F16", "0", "split", 0), ("PMCE_SPLIT_MIN_BATCH", "48", "min_batch", 48),
                                ("PMCE_STRICT_OVERFLOW", "1", "strict", 1), ("PMCE_SINGLE_STREAM", "1", "two_streams", 0),
                                ("PMCE_SPLIT_OVERLAP", "0", "overlap", 0)):
        monkeypatch.setenv(var, val)
        st = create()
        assert st[key] == want and all(st[k] == base[k] for k in st if k != key), (var, st)
        monkeypatch.delenv(var)
    # the API equivalents
    h = C.c_void_p()
    assert lib.pmce_model_create(17, 256, 3, C.byref(h)) == 0
    assert lib.pmce_model_set_split_min_batch(h, 7) == 0 and lib.pmce_model_get_split_min_batch(h) == 7
    assert lib.pmce_model_set_overflow_policy(h, 1) == 0 and lib.pmce_model_get_overflow_policy(h) == 1
    assert lib.pmce_model_set_concurrency(h, 0) == 0 and lib.pmce_model_get_concurrency(h) == 0
    lib.pmce_model_destroy(h)
    # nothing else is read: every getenv / pmce_env_int in the sources names one of the five
    from pmce_amd import build as B
    names = set()
    for f in os.listdir(B.CSRC):
        if f.endswith((".hip", ".cpp", ".hpp")):
            src = open(osp.join(B.CSRC, f)).read()
            names |= set(re.findall(r'(?:getenv|pmce_env_int)\(\s*"([A-Z0-9_]+)"', src))
    assert names == {"PMCE_SPLIT_F16", "PMCE_SPLIT_MIN_BATCH", "PMCE_STRICT_OVERFLOW", "PMCE_SINGLE_STREAM", "PMCE_SPLIT_OVERLAP"}, names


def test_facade_keeps_reference_checkpoint_layout():
    from pmce_amd import _lib, models, synth
    spec = synth.pmce_spec(19, 256, 3)
    m = models.PMCE.get_model(19, 256, 3)
    sd = m.state_dict()
    assert set(sd.keys()) == set(spec.keys()) and len(sd) == len(spec)
    assert all(tuple(sd[k].shape) == tuple(spec[k][0]) for k in spec)
    assert m.vj_relation.shape == (431,) and m.vj_relation.max() <= 16
    assert not m.training
    with pytest.raises(_lib.PmceError):
        m(torch.zeros(1, 16, 19, 2), torch.zeros(1, 16, 2048))     # no CPU fallback
    with pytest.raises(RuntimeError):
        m.load_state_dict({"model_state_dict": {"pose_lifter.joint_embed.weight": torch.zeros(256, 2)}})  # strict
    lifter = models.PoseEstimation.get_model(17, 256, 3)
    assert set(lifter.state_dict().keys()) == set(synth.lifter_spec(17, 256, 3).keys())
    dec = models.CoevoDecoder.get_model(17, 256)
    assert set(dec.state_dict().keys()) == set(synth.decoder_spec(17).keys())


def test_packed_final_product_equals_conv_plus_linears():
    """pack_final: Conv1d(431->6890,k=3,pad=1) + 3 Linear(2048->6890) == one [.,3360] x [3360,20670] product."""
    from oracle import pmce_oracle as O
    from pmce_amd import packing
    sd = cached_state_dict(17, 256)
    W, b = packing.pack_final(sd, "pose_mesh_coevo.", torch.device("cpu"))
    assert W.shape == (20670, packing.FINAL_K) and b.shape == (20670,)
    B = 2
    g = T(np.random.default_rng(0).standard_normal((B, 2048)).astype(np.float32))
    vt = T(np.random.default_rng(1).standard_normal((B, 431, 3)).astype(np.float32))
    A = torch.zeros(B, packing.FINAL_K)
    A[:, :2048] = torch.relu(g)
    A[:, 2048:2048 + 1293] = vt.reshape(B, -1)
    got = (A.double() @ W.double().t() + b.double()).reshape(B, 6890, 3)
    with torch.no_grad():
        ref = O.upsample_and_residual(vt, g, sd, "pose_mesh_coevo.", torch.float64)
    assert float((got - ref).abs().max()) < 1e-6


def test_packed_adaln_and_gru_layout():
    from oracle import pmce_oracle as O
    from pmce_amd import assets, packing
    sd = cached_state_dict(17, 256)
    _, vj, _ = assets.build_template("/nonexistent")
    pk = packing.pack_decoder(sd, "pose_mesh_coevo.", torch.device("cpu"), 17, vj)
    g = T(np.random.default_rng(2).standard_normal((3, 2048)).astype(np.float32))
    GB = g @ pk["dec.ada.weight"].t() + pk["dec.ada.bias"]
    assert GB.shape == (3, packing.N_ADA * 128)
    for i, name in enumerate(packing.ADA_ORDER):
        p = "pose_mesh_coevo." + name
        gam = torch.nn.functional.linear(g, sd[p + ".mlp_gamma.weight"], sd[p + ".mlp_gamma.bias"])
        bet = torch.nn.functional.linear(g, sd[p + ".mlp_beta.weight"], sd[p + ".mlp_beta.bias"])
        assert torch.allclose(GB[:, i * 128:i * 128 + 64], gam, atol=1e-5)
        assert torch.allclose(GB[:, i * 128 + 64:(i + 1) * 128], bet, atol=1e-5)
    assert pk["dec.gru.w_ih_l0"].shape == (6144, 2048) and pk["dec.gru.w_hh_l1"].shape == (2, 3072, 1024)
    assert torch.equal(pk["dec.gru.w_ih_l0"][3072:], sd["pose_mesh_coevo.gru_cur.weight_ih_l0_reverse"])
    assert pk["dec.vj_relation"].dtype == torch.int32
    k3 = "pose_mesh_coevo.coevoblock3."
    eq = sd[k3 + "vertx_proj.bias"][None] + sd[k3 + "vertx_pos_embed"][0] + sd[k3 + "v_Q_embed"][0]
    assert torch.allclose(pk["dec.b3.Eq"], eq, atol=1e-6)
    # every tensor the C model asks for is produced by the packers, and nothing else
    import ctypes as C
    from pmce_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.pmce_model_create(17, 256, 3, C.byref(h)) == 0
    names = {lib.pmce_model_tensor_name(h, i).decode() for i in range(lib.pmce_model_tensor_count(h))}
    lib.pmce_model_destroy(h)
    lk = set(packing.pack_lifter(sd, "pose_lifter.", torch.device("cpu"), 17, 256, 3).keys())
    assert names == lk | set(pk.keys()), names ^ (lk | set(pk.keys()))


def test_regressor_csr_roundtrip():
    from pmce_amd import assets
    for name, nnz in (("h36m", 107), ("coco", 105)):
        jr = assets.load_j_regressor(name)
        indptr, indices, data = assets.regressor_to_csr(jr)
        assert jr.shape == (17, 6890) and len(data) == nnz and indptr[-1] == nnz
        dense = np.zeros_like(jr, dtype=np.float32)
        for r in range(17):
            dense[r, indices[indptr[r]:indptr[r + 1]]] = data[indptr[r]:indptr[r + 1]]
        assert np.array_equal(dense, jr.astype(np.float32))


def test_build_verts_joints_relation_ties_first_index():
    from pmce_amd import assets
    joints = np.array([[0, 0, 0], [2, 0, 0], [0, 0, 0]], dtype=np.float32)       # joint 2 duplicates joint 0
    verts = np.array([[0.1, 0, 0], [1.0, 0, 0], [1.9, 0, 0]], dtype=np.float32)  # middle vertex equidistant
    assert assets.build_verts_joints_relation(joints, verts).tolist() == [0, 0, 1]


def test_checkpoint_tooling(tmp_path):
    from pmce_amd import checkpoint
    sd = cached_state_dict(17, 256)
    p = tmp_path / "mesh_test.pth.tar"
    torch.save({"epoch": 3, "model_state_dict": {"module." + k: v for k, v in sd.items()}, "optim_state_dict": {},
                "scheduler_state_dict": {}, "train_log": [], "test_log": []}, p)          # main/train.py:57-64 format
    sd2, kind, J, C, depth = checkpoint.load_reference_checkpoint(str(p))
    assert (kind, J, C, depth) == ("pmce", 17, 256, 3) and set(sd2) == set(sd)
    lifter = {k[len("pose_lifter."):]: v for k, v in sd.items() if k.startswith("pose_lifter.")}
    assert checkpoint.infer_dims(lifter) == ("lifter", 17, 256, 3)
    bad = dict(sd)
    bad.pop("pose_lifter.norm_s.weight")
    bad["pose_mesh_coevo.linear_cur1.bias"] = torch.zeros(5)
    bad["extra.key"] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        checkpoint.validate_state_dict(bad)
    msg = str(e.value)
    assert "missing: pose_lifter.norm_s.weight" in msg and "shape: pose_mesh_coevo.linear_cur1.bias" in msg and "unexpected: extra.key" in msg
    with pytest.raises(ValueError, match="No checkpoint exists"):
        checkpoint.load_reference_checkpoint(str(tmp_path / "nope.pth.tar"))


def test_checkpoint_written_like_the_reference_training_loop(tmp_path):
    """What main/train.py:57-64 really saves: the error logs hold NUMPY scalars (compute_both_err's np.power(...).mean()), the
    optimizer state is Adam's, the scheduler's is a MultiStepLR's with its Counter of milestones.  The restricted unpickler
    must take such a file (round 2's plain weights_only=True did not), refuse a file that carries anything executable, say
    what went wrong, and leave the unrestricted unpickler as an explicit opt-in - also for GraphormerNet(pretrained=True)."""
    from pmce_amd import checkpoint, models, synth
    from pmce_amd.config import cfg
    sd = cached_state_dict(17, 256)
    lifter = {k[len("pose_lifter."):]: v for k, v in sd.items() if k.startswith("pose_lifter.")}
    net = torch.nn.Linear(4, 4)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    net(torch.zeros(1, 4)).sum().backward()
    opt.step()
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[2, 4], gamma=0.1)
    logs = [np.float32(101.5), np.float64(88.25), np.power(np.ones(3, np.float32) * 2, 2).mean()]
    p = tmp_path / "pose_best.pth.tar"
    torch.save({"epoch": 7, "model_state_dict": lifter, "optim_state_dict": opt.state_dict(),
                "scheduler_state_dict": sched.state_dict(), "train_log": logs, "test_log": list(logs)}, p)
    sd2, kind, J, C, depth = checkpoint.load_reference_checkpoint(str(p))
    assert (kind, J, C, depth) == ("lifter", 17, 256, 3) and all(torch.equal(sd2[k], lifter[k]) for k in lifter)
    obj = checkpoint.torch_load_checkpoint(str(p))
    assert obj["epoch"] == 7 and float(obj["test_log"][1]) == 88.25 and obj["scheduler_state_dict"]["milestones"][2] == 1
    cfg.MODEL.posenet_path = str(p)
    try:
        m = models.PoseEstimation.get_model(17, 256, 3, pretrained=True)
        assert torch.equal(m.state_dict()["norm_s.weight"], lifter["norm_s.weight"])
    finally:
        cfg.MODEL.posenet_path = ""

    class Evil:      # something the allow-list does not know
        def __reduce__(self):
            return (print, ("code ran while unpickling",))
    q = tmp_path / "evil.pth.tar"
    torch.save({"model_state_dict": lifter, "extra": Evil()}, q)
    with pytest.raises(ValueError) as e:
        checkpoint.load_reference_checkpoint(str(q))
    assert "No checkpoint exists" in str(e.value) and "allow_pickle=True" in str(e.value) and "UnpicklingError" in str(e.value)
    sd3 = checkpoint.load_reference_checkpoint(str(q), allow_pickle=True)[0]
    assert set(sd3) == set(lifter)


def test_checkpoint_loader_on_a_torch_without_safe_globals(tmp_path, monkeypatch):
    """torch < 2.5 has no ``torch.serialization.safe_globals``: the loader must use ``add_safe_globals`` (2.4) or say that this
    torch cannot read a reference checkpoint restricted - not swallow an AttributeError into "the file holds objects outside ..."
    and not fall through to the unrestricted unpickler for an unrelated failure."""
    from pmce_amd import checkpoint
    sd = cached_state_dict(17, 256)
    lifter = {k[len("pose_lifter."):]: v for k, v in sd.items() if k.startswith("pose_lifter.")}
    p = tmp_path / "pose.pth.tar"
    torch.save({"epoch": 1, "model_state_dict": lifter, "test_log": [np.float64(1.5)]}, p)
    ser = torch.serialization
    monkeypatch.delattr(ser, "safe_globals")                 # "torch 2.4"
    assert checkpoint.load_reference_checkpoint(str(p))[1] == "lifter"
    monkeypatch.delattr(ser, "add_safe_globals")             # "torch < 2.4"
    with pytest.raises(ValueError) as e:
        checkpoint.load_reference_checkpoint(str(p))
    assert "no allow-list" in str(e.value) and "holds objects outside" not in str(e.value)
    assert checkpoint.load_reference_checkpoint(str(p), allow_pickle=True)[1] == "lifter"
    monkeypatch.undo()
    # an unrelated failure (a truncated file) is reported as what it is and never retried with the unrestricted unpickler
    q = tmp_path / "cut.pth.tar"
    q.write_bytes(p.read_bytes()[:2000])
    calls = []
    real = torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: (calls.append(k.get("weights_only")), real(*a, **k))[1])
    with pytest.raises(ValueError):
        checkpoint.load_reference_checkpoint(str(q), allow_pickle=True)
    assert calls == [True]


def test_workload_flops_match_the_survey_split():
    """The analytical work bench.py divides times into, against SURVEY §8d's per-module figures (its FlopCounter probe of the REFERENCE forward
    at J = 17, C = 256): lifter 1.756e9, GRU 1.208e9, three CoevoBlocks + the 72 AdaLN Linear layers 0.449e9, upsample conv 0.0535e9 +
    residual Linear layers 0.0847e9, total 3.552e9 - each to the survey's printed precision."""
    from pmce_amd.workload import flops_per_clip
    f = flops_per_clip(17, 256)
    assert abs(f["lifter"] - 1.756e9) < 1.5e6
    assert abs(f["gru"] - 1.208e9) < 0.5e6
    assert abs(f["coevo"] - 0.449e9) < 1.0e6
    assert abs(f["upsample"] - (0.0535e9 + 0.0847e9)) < 0.2e6
    assert abs(f["total"] - 3.552e9) < 2e6 and f["total"] == f["lifter"] + f["gru"] + f["coevo"] + f["upsample"]
    # scaling laws of the architecture: the GRU and the decoder do not depend on the pose-encoder width; the lifter's products are
    # quadratic in it
    g = flops_per_clip(17, 512)
    assert g["gru"] == f["gru"] and g["coevo"] == f["coevo"] and g["upsample"] == f["upsample"] and 3.5 < g["lifter"] / f["lifter"] < 4.0


def test_workspace_size_is_monotonic_in_batch(lib):
    """the fused self-attention's scratch took two tile sets per clip up to B = 128 and one beyond, which made
    pmce_model_workspace_bytes(129) < (128): a caller sizing once for its largest batch (C API), or HipEngine.workspace growing by batch
    count, then failed check_ws on a smaller batch.  The size is non-decreasing now and the engine compares bytes."""
    import ctypes as C
    assert [lib.pmce_vertex_sab_scratch_floats(b) for b in (128, 129, 256, 257)] == sorted(lib.pmce_vertex_sab_scratch_floats(b) for b in (128, 129, 256, 257))
    for J, Cw in ((17, 256), (19, 512)):
        h = C.c_void_p()
        assert lib.pmce_model_create(J, Cw, 3, C.byref(h)) == 0
        sizes = [lib.pmce_model_workspace_bytes(h, b) for b in range(1, 400)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), [i + 1 for i, (a, b) in enumerate(zip(sizes, sizes[1:])) if b < a]
        lib.pmce_model_destroy(h)


def test_synthetic_template_is_opt_in(monkeypatch):
    """a missing smpl_mean_vertices.npy / mesh_downsampling.npz must raise (vj_relation is derived from them and
    is not in the checkpoint); the synthetic stand-ins are an explicit opt-in."""
    from pmce_amd import assets, models
    monkeypatch.setenv("PMCE_SYNTHETIC_BASE_DATA", "0")
    assets.allow_synthetic_base_data(False)
    with pytest.raises(FileNotFoundError):
        assets.build_template("/nonexistent")
    with pytest.raises(FileNotFoundError):
        models.PMCE.get_model(17, 256, 3)
    assets.allow_synthetic_base_data(True)
    try:
        assert assets.build_template("/nonexistent")[2] == "synthetic"
    finally:
        assets.allow_synthetic_base_data(False)
    monkeypatch.setenv("PMCE_SYNTHETIC_BASE_DATA", "1")
    assert assets.build_template("/nonexistent")[2] == "synthetic"


def test_window_tables_are_validated():
    from pmce_amd import streaming
    ok = streaming.validate_windows(streaming.demo_window_list(40), 40)
    assert ok.dtype == np.int32 and ok.shape == (40, 2)
    assert streaming.validate_windows(np.zeros((0, 2)), 10).shape == (0, 2)
    for bad, L in (([[0, 15]], 15),            # runs past the sequence
                   ([[-1, 14]], 40),           # negative start
                   ([[3, 10]], 40),            # neither 16 consecutive frames nor a repeated frame
                   ([[9, 2]], 40)):            # start > end
        with pytest.raises(ValueError):
            streaming.validate_windows(bad, L)
    with pytest.raises(ValueError):            # demo list of a sequence shorter than one window
        streaming.demo_window_list(10)


def test_checkpoint_loading_does_not_unpickle_code(tmp_path):
    """reference-style checkpoint dicts load with weights_only=True; a file that needs the unrestricted unpickler is
    refused unless the caller opts in."""
    import torch
    from pmce_amd import checkpoint, synth
    sd = synth.make_state_dict(synth.lifter_spec(17, 256, 3), seed=1)
    f = tmp_path / "pose.pth.tar"
    torch.save({"epoch": 3, "model_state_dict": {"module." + k: v for k, v in sd.items()}}, f)
    got, kind, J, C, depth = checkpoint.load_reference_checkpoint(str(f))
    assert (kind, J, C, depth) == ("lifter", 17, 256, 3) and set(got) == set(sd)

    class Evil:
        def __reduce__(self):
            return (print, ("code ran while unpickling",))

    g = tmp_path / "evil.pth.tar"
    torch.save({"model_state_dict": sd, "extra": Evil()}, g)
    with pytest.raises(ValueError):
        checkpoint.load_reference_checkpoint(str(g))


def test_bench_roofline_arithmetic():
    """bench.py's analytical side (no GPU): work per kernel class and the two floors of the north-star kernel."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", osp.join(REPO, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B, J = 256, 17
    # the four lifter products of one block at C = 512: 2*M*K*(3C + C + 2C + 2C) with M = B*16*J
    M = B * 16 * J
    per_block = 2.0 * M * 512 * (1536 + 512 + 1024 + 1024)
    assert bench.gemm_lifter_flops(B, J, 512) == 2.0 * B * 16 * 2048 * 512 + 6 * per_block
    w, kind = bench.class_work("vertex_ca", B, J, 512)
    assert kind == "byte" and w == 3 * 229376.0 * B
    rec = bench.north_star_record({"vertex_ca_mlp": 0.345, "adaln_mlp": 0.27}, {"vertex_ca_mlp": 3, "adaln_mlp": 3}, B, J)
    # 14 wave tiles per clip, (64 + 16*ceil(17/8) + 512) MFMAs of 64 cycles each, 1024 SIMDs at 2.4 GHz
    assert abs(rec["mfma_floor_ms"] - B * 14 * 624 * 64 / 1024 / 2.4e9 * 1e3) < 1e-5
    assert abs(rec["hbm_floor_ms"] - 229376.0 * B / 8e12 * 1e3) < 1e-5
    assert rec["kernel"] == "vertex_ca_mlp" and rec["bound"] == "mfma" and abs(rec["frac_of_floor"] - rec["mfma_floor_ms"] / 0.115) < 1e-3
    rec16 = bench.north_star_record({"vertex_ca_mlp": 0.18}, {"vertex_ca_mlp": 3}, B, J, f16_ffn=True)
    # split-f16 mode: 24 score + 12 * ceil(17/16) output + 192 FFN matrix instructions of 32 cycles per wave tile
    assert abs(rec16["mfma_floor_ms"] - B * 14 * (24 + 24 + 192) * 32 / 1024 / 2.4e9 * 1e3) < 1e-5
    old = bench.north_star_record({"vertex_ca": 0.09}, {"vertex_ca": 3}, B, J)
    assert old["kernel"] == "vertex_ca" and abs(old["mfma_floor_ms"] - B * 14 * 112 * 64 / 1024 / 2.4e9 * 1e3) < 1e-5
    assert bench.north_star_record({"gemm_lifter": 1.0}, {"gemm_lifter": 25}, B, J) is None


def test_hot_kernels_do_not_spill(lib, tmp_path):
    """The kernels of the default (split-f16) path keep everything in registers: no VGPR spills, no scratch (the packed-output GEMM
    epilogue once fell to 59 spilled registers after an unrelated change and cost 12 % of the headline without failing a test).
    Read from the code objects' metadata notes.  Known exception, outside the default path: the vector-pipe attention the fp32 mode uses at
    C = 512."""
    import shutil
    import subprocess
    from pmce_amd import build as B
    B.build()
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (osp.exists(objdump) and osp.exists(readelf)):
        pytest.skip("llvm-objdump / llvm-readelf not available")
    allowed = ("seq_attention_pair_kernel", "sample_errors_kernel")   # (metrics: a private array by design)
    seen = 0
    for src in ("gemm_split_f16.hip", "gemm_f32.hip", "gemm_f16.hip", "seq_attention_mfma.hip", "vit_attention.hip", "conv.hip", "yolo.hip",
                "lifter.hip", "gru.hip", "coevo.hip"):
        obj = osp.join(B.CSRC, "build", osp.splitext(src)[0] + ".o")
        if not osp.exists(obj):
            pytest.skip(f"{obj} not present (library built elsewhere)")
        local = str(tmp_path / osp.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([objdump, "--offloading", local], check=True, capture_output=True, cwd=str(tmp_path))
        dev = [f for f in os.listdir(tmp_path) if f.startswith(osp.basename(obj) + ".") and "amdgcn" in f]
        assert dev, f"no device code object extracted from {obj}"
        notes = subprocess.run([readelf, "--notes", str(tmp_path / dev[0])], check=True, capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1))
            scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            seen += 1
            if any(a in name for a in allowed):
                continue
            assert spills == 0 and scratch == 0, f"{src}: {name} spills {spills} VGPRs / uses {scratch} B of scratch"
    assert seen > 60
