"""Host test of the networks' shared finalize (csrc/net_weights.cpp): a finalize that failed leaves the handle as it was, so it can be
called again.  Without a device the allocation of the arena is the step that fails; the tensors' pointers are never read."""
import ctypes as C

import pytest
import torch

import yolo_ref as YR
from pmce_amd import yolo as Y

FAKE = 256          # a non-null, 16-byte aligned "device pointer"


@pytest.fixture(scope="module")
def lib():
    from pmce_amd import _lib, build
    build.build()
    if torch.cuda.is_available():
        pytest.skip("with a device the allocation succeeds and finalize would read the made-up pointers")
    return _lib.load()


def _extractor(lib):
    h = C.c_void_p()
    assert lib.pmce_extractor_create(C.byref(h)) == 0
    for i in range(lib.pmce_extractor_conv_count(h)):
        assert lib.pmce_extractor_set_conv(h, lib.pmce_extractor_conv_name(h, i), FAKE, FAKE) == 0
    return h


def _vitpose(lib):
    h = C.c_void_p()
    assert lib.pmce_vitpose_create(64, 48, 128, 1, 2, 32, 32, 17, C.byref(h)) == 0
    for i in range(lib.pmce_vitpose_tensor_count(h)):
        assert lib.pmce_vitpose_set_tensor(h, lib.pmce_vitpose_tensor_name(h, i), FAKE) == 0
    return h


def _yolo(lib):
    spec = YR.mini_spec()
    h = Y._create(spec)
    for i, _, _, _, _ in Y.conv_table(spec):
        assert lib.pmce_yolo_set_conv(h, i, FAKE, FAKE) == 0
    return h


@pytest.mark.parametrize("net,make", [("extractor", _extractor), ("vitpose", _vitpose), ("yolo", _yolo)])
def test_finalize_can_be_called_again_after_it_failed(lib, net, make):
    from pmce_amd import _lib
    h = make(lib)
    finalize, destroy = getattr(lib, f"pmce_{net}_finalize_on"), getattr(lib, f"pmce_{net}_destroy")
    for _ in range(2):
        assert finalize(h, None) == -3, _lib.last_error()                 # PMCE_ERR_WORKSPACE, not "already finalized"
        assert f"{net}_finalize: hipMalloc" in _lib.last_error()
    destroy(h)
