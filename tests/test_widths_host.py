"""CPU-only tests of the lifter widths: pmce_model_create takes embed_dim 128, 256, 384 and 512 (a multiple of 128 from 128 to 512) and
states that rule when it refuses; the attention entry pair that serves every accepted width is declared, prototyped and exported, and
refuses what it does not serve before any launch; the workspace size stays monotonic at the new widths; the checkpoint reader infers them."""
import ctypes as C
import os.path as osp
import re

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    return _lib.load()


@pytest.mark.parametrize("width", [128, 256, 384, 512])
def test_model_create_accepts_the_four_widths(lib, width):
    h = C.c_void_p()
    assert lib.pmce_model_create(17, width, 3, C.byref(h)) == 0
    names = [lib.pmce_model_tensor_name(h, i).decode() for i in range(lib.pmce_model_tensor_count(h))]
    assert "lifter.SpatialBlocks.2.mlp.fc2.bias" in names
    assert lib.pmce_model_workspace_bytes(h, 3) > 0
    lib.pmce_model_destroy(h)


@pytest.mark.parametrize("width", [64, 192, 300, 320, 448, 640, 0, -128])
def test_model_create_refuses_other_widths_and_states_the_rule(lib, width):
    from pmce_amd import _lib
    h = C.c_void_p()
    assert lib.pmce_model_create(17, width, 3, C.byref(h)) == -1
    msg = _lib.last_error()
    assert "multiple of 128 from 128 to 512" in msg and f"got {width}" in msg, msg


def test_new_attention_entries_are_declared_prototyped_and_exported(lib):
    from pmce_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(osp.join(REPO, "include", "pmce_hip.h")).read(), flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ("pmce_lifter_attention_f32", "pmce_lifter_attention_split_supported", "pmce_lifter_attention_split_f16"):
        m = re.search(r"\b" + name + r"\s*\(([^)]*)\)", hdr)
        assert m, f"{name} is not declared in include/pmce_hip.h"
        nargs = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name]) == nargs, (name, nargs)
        assert hasattr(raw, name)
    # the entries take what the existing entries take: the same argument lists
    assert _lib.PROTOTYPES["pmce_lifter_attention_f32"] == _lib.PROTOTYPES["pmce_seq_attention_f32"]
    assert _lib.PROTOTYPES["pmce_lifter_attention_split_f16"] == _lib.PROTOTYPES["pmce_seq_attention_split_f16"]
    assert _lib.PROTOTYPES["pmce_lifter_attention_split_supported"] == _lib.PROTOTYPES["pmce_seq_attention_split_supported"]


def test_new_attention_entry_validates_on_the_host(lib):
    from pmce_amd import _lib
    for Cw in (128, 256, 384, 512):
        for N in (16, 17, 19):
            assert lib.pmce_lifter_attention_split_supported(N, Cw) == 1
        for N in (1, 15, 18, 24, 32):
            assert lib.pmce_lifter_attention_split_supported(N, Cw) == 0
    for Cw in (64, 192, 320, 448, 640):
        assert lib.pmce_lifter_attention_split_supported(17, Cw) == 0
    # the existing entries keep their contract
    assert lib.pmce_seq_attention_split_supported(17, 384) == 0 and lib.pmce_seq_attention_split_supported(17, 128) == 0
    assert lib.pmce_seq_attention_f32(16, 16, 4, 17, 384, 0, 17, 0, 1, 0, None) == -1 and "256 or 512" in _lib.last_error()
    # refused before any launch (no GPU here: a launch would not return -1 with this text)
    for N, Cw in ((24, 384), (17, 192), (24, 512)):
        rc = lib.pmce_lifter_attention_split_f16(16, 16, 4, N, Cw, 0, N, 0, 1, None)
        assert rc == -1 and "16, 17 or 19" in _lib.last_error() and f"N={N} C={Cw}" in _lib.last_error()
    assert lib.pmce_lifter_attention_split_f16(None, 16, 4, 17, 384, 0, 17, 0, 1, None) == -1
    assert lib.pmce_lifter_attention_split_f16(16, 16, 0, 17, 384, 0, 17, 0, 1, None) == -1
    assert lib.pmce_lifter_attention_split_f16(16, 16, 4, 17, 384, 0, 17, 0, 0, None) == -1     # token stride 0


def test_row_kernel_entries_refuse_other_widths_on_the_host(lib):
    from pmce_amd import _lib
    for Cw in (64, 192, 320, 640):
        assert lib.pmce_ln_chain_f32(16, 4, Cw, None, None, 0.0, None, 1, 1, 16, None, None, 0.0, None, 0, None) == -1
        assert f"got {Cw}" in _lib.last_error()
        assert lib.pmce_lifter_attention_f32(16, 16, 4, 17, Cw, 0, 17, 0, 1, 0, None) == -1
        assert "128, 256, 384 or 512" in _lib.last_error() and f"got {Cw}" in _lib.last_error()
        assert lib.pmce_lifter_head_f32(16, None, None, 0.0, 16, 16, 16, 16, 16, 16, 16, 1, 16, 17, Cw, None) == -1
    assert lib.pmce_lifter_attention_f32(16, 16, 4, 33, 384, 0, 33, 0, 1, 0, None) == -1 and "1..32" in _lib.last_error()


def test_workspace_size_is_monotonic_in_batch_at_the_new_widths(lib):
    for J, Cw in ((17, 128), (19, 384)):
        h = C.c_void_p()
        assert lib.pmce_model_create(J, Cw, 3, C.byref(h)) == 0
        sizes = [lib.pmce_model_workspace_bytes(h, b) for b in range(1, 400)]
        assert all(s > 0 for s in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), [i + 1 for i, (a, b) in enumerate(zip(sizes, sizes[1:])) if b < a]
        lib.pmce_model_destroy(h)


@pytest.mark.parametrize("J,Cw", [(17, 128), (19, 384)])
def test_checkpoint_infers_the_new_widths(J, Cw):
    from pmce_amd import checkpoint, packing, synth, workload
    sd = synth.make_state_dict(synth.pmce_spec(J, Cw, 2), seed=5)
    assert checkpoint.infer_dims(sd) == ("pmce", J, Cw, 2)
    assert checkpoint.validate_state_dict(sd) == ("pmce", J, Cw, 2)
    lsd = synth.make_state_dict(synth.lifter_spec(J, Cw, 3), seed=5)
    assert checkpoint.infer_dims(lsd) == ("lifter", J, Cw, 3)
    assert packing.expected_shapes(J, Cw, 2)["pose_lifter.spatial_pos_embed"] == (1, J, Cw)
    # the lifter's products are quadratic in the width, the rest of the path does not depend on it
    f, g = workload.flops_per_clip(J, Cw), workload.flops_per_clip(J, 2 * Cw if Cw == 128 else 512)
    assert f["gru"] == g["gru"] and f["coevo"] == g["coevo"] and f["lifter"] < g["lifter"]
