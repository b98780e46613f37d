"""The settings a multi-rank transport is created with (comm_mp_settings.cc
mpSettings), on the CPU through nbxDebugTransportSettings: the function
ncclCommInitRank and ncclCommInitAll run before they allocate anything, here
on given rank counts and CU counts under each case's environment.

Expected values: what tests/test_multiprocess_gpu.py's knob tests state
(test_multiprocess_reference_knobs, _config_ctas, _nbx_override_wins, the plan
checks), and for every other case what the library before this function
existed reported from nbxDebugCommSettings / nbxDebugCommProtoMask on an
MI355X — profiles/r13/records_parent.txt, written by
scripts/mp_creation_records.py, whose case list this test replays. That run had
256 CUs and every rank on one GPU: minCus = 256, maxShare = the rank count,
multiGpu = 0. NCCL_MAX_CTAS and NCCL_CHECK_POINTERS reach mpSettings through
the communicator (nccl_api.cc newComm), so the test passes them as inputs."""
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDEF = -2 ** 31   # NCCL_CONFIG_UNDEF_INT
K, M = 1 << 10, 1 << 20
CUS = 256          # the MI355X of profiles/r13


def _records_tool():
    spec = importlib.util.spec_from_file_location("mp_creation_records",
                                                  os.path.join(ROOT, "scripts", "mp_creation_records.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _records_tool()


@pytest.fixture(scope="module")
def lib(nbx):
    lib = nbx.load_library()
    lib.nbxDebugTransportSettings.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
    lib.nbxDebugTransportSettings.restype = ctypes.c_int
    return lib


def _settings(lib, n, min_cus=CUS, max_share=None, multi=0, min_ctas=UNDEF, max_ctas=UNDEF, check_pointers=0):
    out = (ctypes.c_int64 * 16)()
    got = lib.nbxDebugTransportSettings(n, min_cus, n if max_share is None else max_share, multi, min_ctas, max_ctas,
                                        check_pointers, out, 16)
    assert got == 16
    return list(out)


def _clean(monkeypatch):
    for k in TOOL.KNOBS:
        monkeypatch.delenv(k, raising=False)


def _slot_lines(ll_max, l128_max):
    """LL: 2 lines per 8-byte pack; LL128: two halves of ceil(max / 2 / 48) 64-byte lines (48 payload bytes)."""
    return 2 * (ll_max // 8), 2 * -(-((l128_max + 1) // 2) // 48)


def test_defaults_named_in_the_comments(lib, monkeypatch):
    """No knob set, a GPU per rank: 64 KiB LL, 1 MiB LL128 (one-shot to 256 KiB), 64 KiB slices in
    2 slots, 128 Simple workgroups, LL / LL128 grids of 4 / 1 per CU, group batching on, checks
    off, every protocol, direct schedule."""
    _clean(monkeypatch)
    assert _settings(lib, 2, min_cus=CUS, max_share=1) == [
        64 * K, 1 * M, 64 * K, 2, 128, 4 * CUS, CUS, 1, 0, 0, 0, 7, 0, 256 * K, 16384, 21846]
    # across GPUs LL128 leaves the default set; past 8 ranks there is no LL128 at all
    assert _settings(lib, 2, max_share=1, multi=1)[11] == 5
    nine = _settings(lib, 9, max_share=1)
    assert (nine[1], nine[13], nine[15]) == (0, 0, 0) and nine[0] == 64 * K


def test_bad_inputs(lib):
    out = (ctypes.c_int64 * 16)()
    for args in [(1, CUS, 1), (65, CUS, 1), (2, 0, 1), (2, CUS, 0)]:
        assert lib.nbxDebugTransportSettings(*args, 0, UNDEF, UNDEF, 0, out, 16) == -1
    assert lib.nbxDebugTransportSettings(2, CUS, 1, 0, UNDEF, UNDEF, 0, None, 16) == -1
    assert lib.nbxDebugTransportSettings(2, CUS, 1, 0, UNDEF, UNDEF, 0, out, 3) == 3


REF = {"NCCL_LL_BUFFSIZE": "65536", "NCCL_LL128_BUFFSIZE": "1048576", "NCCL_MAX_NCHANNELS": "16"}


@pytest.mark.parametrize("buffsize,slice_want", [("65536", 32768), ("4194304", 65536)])
def test_reference_knobs(lib, monkeypatch, buffsize, slice_want):
    """test_multiprocess_reference_knobs' arithmetic: 32768 / 786432 / slice / 2 / 16, every grid capped at 16."""
    _clean(monkeypatch)
    for k, v in dict(REF, NCCL_BUFFSIZE=buffsize).items():
        monkeypatch.setenv(k, v)
    assert _settings(lib, 2) == [32768, 786432, slice_want, 2, 16, 16, 16, 1, 0, 0, 0, 7, 0, 256 * K,
                                 *_slot_lines(32768, 786432)]


@pytest.mark.parametrize("cfg,env,grid", [({"max_ctas": 8}, {}, 8), ({"min_ctas": 16, "max_ctas": 64}, {}, 64),
                                          ({"max_ctas": 4}, {}, 4),     # maxCTAs 64 under NCCL_MAX_CTAS=4: newComm
                                          ({"max_ctas": 100}, {"NCCL_MAX_NCHANNELS": "12"}, 12)])
def test_config_ctas(lib, monkeypatch, cfg, env, grid):
    """test_multiprocess_config_ctas' four grids; 128 CUs per rank never bind below them."""
    _clean(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _settings(lib, 2, **cfg) == [64 * K, 1 * M, 64 * K, 2, grid, grid, grid, 1, 0, 0, 0, 7, 0, 256 * K,
                                        16384, 21846]


def test_nbx_override_wins(lib, monkeypatch):
    """test_multiprocess_nbx_override_wins: slice 16384 and grid 6; NCCL_MAX_NCHANNELS=4 still caps LL / LL128."""
    _clean(monkeypatch)
    for k, v in {"NCCL_BUFFSIZE": "262144", "NBX_SIMPLE_SLICE_BYTES": "16384", "NCCL_MIN_NCHANNELS": "8",
                 "NCCL_MAX_NCHANNELS": "4", "NBX_SIMPLE_MAX_GRID": "6"}.items():
        monkeypatch.setenv(k, v)
    assert _settings(lib, 2) == [64 * K, 1 * M, 16384, 2, 6, 4, 4, 1, 0, 0, 0, 7, 0, 256 * K, 16384, 21846]


def _recorded():
    """{case name: (settings, mask)} of rank 0 of every multi-process case the parent created."""
    out = {}
    with open(os.path.join(ROOT, "profiles", "r13", "records_parent.txt")) as f:
        for line in f:
            head, body = line.split(": ", 1)
            rec = json.loads(body)
            if head.endswith(" rank 0") and "settings" in rec:
                out[head[:-len(" rank 0")]] = (rec["settings"], rec["mask"])
    return out


RECORDED = _recorded()
MP_CASES = [c for c in TOOL.CASES if not c[4] and not c[0].startswith("differ-")]


def test_every_recorded_case_is_replayed():
    assert sorted(RECORDED) == sorted(c[0] for c in MP_CASES) and len(MP_CASES) == 22


@pytest.mark.parametrize("case", MP_CASES, ids=[c[0] for c in MP_CASES])
def test_recorded_case(lib, monkeypatch, case):
    """Slots 0-10 (re-exports aside: mpConnect's) and the protocol mask as the parent's communicator
    reported them on the GPU; ring, one-shot max and slot lines from the case's own knobs."""
    name, n, env, cfg, _ = case
    _clean(monkeypatch)
    env = {k: v[0] for k, v in env.items()}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg = dict(cfg or {})
    if "NCCL_MAX_CTAS" in env:   # envConfigOverride, applied by newComm
        cfg["maxCTAs"] = int(env["NCCL_MAX_CTAS"])
    got = _settings(lib, n, min_ctas=cfg.get("minCTAs", UNDEF), max_ctas=cfg.get("maxCTAs", UNDEF),
                    check_pointers=int(env.get("NCCL_CHECK_POINTERS", "0")))
    want, mask = RECORDED[name]
    assert got[:8] + got[9:11] == want[:8] + want[9:11] and got[8] == 0, (got, want)
    assert got[11] == mask
    assert got[12] == int(env.get("NCCL_ALGO") == "Ring") and got[13] == 256 * K
    assert tuple(got[14:16]) == _slot_lines(want[0], want[1])
