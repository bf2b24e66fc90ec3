"""The device check and the per-thread error string are one piece of host code shared by every translation unit with entry
points (jtk_amd/csrc/host_common.h).  One entry of each family, given otherwise valid minimal arguments and the first device
ordinal that does not exist, returns JTK_ERR_NO_DEVICE with a message, and the next valid call on the thread clears it.  No
kernel is launched: the calls fail before any device work, and the valid call is the creation of an empty session."""
import ctypes as C

import numpy as np
import pytest

import helpers
from jtk_amd import api, ffi

pytestmark = pytest.mark.gpu

NO_DEVICE = -2


@pytest.fixture(scope="module")
def beyond(jtk_lib):
    """hipGetDeviceCount() of the HIP runtime the library itself is bound to: the first ordinal that is not a device"""
    assert jtk_lib.jtk_lc_device_ok(0) == 1, "needs a gfx950 device"
    with open("/proc/self/maps") as maps:
        path = next(line.split()[-1] for line in maps if "libamdhip64" in line)
    n = C.c_int(0)
    assert C.CDLL(path).hipGetDeviceCount(C.byref(n)) == 0 and n.value >= 1
    return n.value


def _session_create(device):
    b, _, p = helpers.small_batch(n_chunks=1, tmpl_len=200, reads_per_hap=4)
    api.Session(p, b, device=device).close()


def _cluster_features(device):
    _, _, p = helpers.small_batch(n_chunks=1, tmpl_len=200, reads_per_hap=4)
    fc = np.zeros(1, dtype=ffi.FEATURE_CHUNK_DT)
    fc["copy_num"], fc["n_reads"], fc["dim"], fc["local_coverage"] = 2, 2, 1, 1.0
    api.cluster_features(p, fc, np.array([1.0, -1.0]), np.zeros(2, np.uint32), 2, device=device)


def _estimate_gains(device):
    api.estimate_gains(ffi.default_hmm(), ffi.default_hmm(), device=device)


def _correct_clustering(device):
    nodes = np.zeros(1, dtype=ffi.CC_NODE_DT)
    nodes["is_forward"], nodes["post_len"] = 1, 1
    chunks = np.zeros(1, dtype=ffi.CC_CHUNK_DT)
    chunks["cluster_num"], chunks["copy_num"] = 1, 1
    api.correct_clustering([0], [0, 1], nodes, [0.0], chunks, [0], 10.0, 1.0, device=device)


def _align_reads(device):
    b, _, _ = helpers.small_batch(n_chunks=1, tmpl_len=200, reads_per_hap=4)
    api.align_reads(b, device=device)


@pytest.mark.parametrize("entry", [_session_create, _cluster_features, _estimate_gains, _correct_clustering, _align_reads],
                         ids=lambda f: f.__name__.lstrip("_"))
def test_an_ordinal_beyond_the_devices_is_a_status_and_the_next_call_clears_it(jtk_lib, beyond, entry):
    with pytest.raises(ffi.JtkError) as e:
        entry(beyond)
    assert e.value.status == NO_DEVICE
    assert jtk_lib.jtk_lc_last_error() != b""
    _, _, p = helpers.small_batch(n_chunks=1, tmpl_len=200, reads_per_hap=4)
    h = C.c_void_p()
    assert jtk_lib.jtk_lc_session_create(C.byref(p), 0, None, None, None, None, None, None, None, 1, 0, C.byref(h)) == 0
    assert jtk_lib.jtk_lc_last_error() == b""
    assert jtk_lib.jtk_lc_session_destroy(h) == 0
