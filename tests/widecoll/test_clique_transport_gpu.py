"""Wide (fp32-accumulating) sums on an in-process clique of 3 ranks sharing the
GPU (ncclCommInitAll) and on a one-rank communicator. A fresh child process per
test (tests/widecoll/worker.py over tests/clique/worker.py's rig, with
tests/clique/cases.CHILD_ENV in its environment before HIP loads).

  fold     the event-ordered fold path: runCliqueColl calls the wide core, so
           every rank's fold leaves a record of families 6 / 7, never 1-3;
  kernel   NBX_CLIQUE_LL=1, the in-kernel transport: an LL clique (family 8)
           and a Simple one (family 11), flags bit 1;
  onerank  nbxRedOpCreateWide's checks on a live handle, create / destroy /
           reuse of a slot, the datatype mismatch at the call, and wide Avg in
           place and out of place as a copy.

Wide Sum / Avg AllReduce, ReduceScatter and Reduce of 5,003 bf16 and fp8
elements, bit for bit against tests/widecoll/cases.py's expectation.

The file carries the name of tests/test_clique_transport_gpu.py on purpose: the
GPU suite orders files by name (tests/conftest.py GPU_FILE_ORDER), and a name
of its own would run between the two groups of tests/test_configs_gpu.py
(tests/test_mp_diag_cpu.py asserts that no file is split)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from tests.clique import cases as clique_cases
from tests.matrix import inputs as mi
from tests.widecoll import cases
from tests.widecoll import worker as ww

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WORKER = os.path.join(ROOT, "tests", "widecoll", "worker.py")
LIMIT = 60   # seconds: a bound for a child that hangs, several times what one takes
GUARD = ww.GUARD


def _run(tmp_path, mode):
    out_file = tmp_path / f"{mode}.pkl"
    env = {k: v for k, v in os.environ.items() if k not in clique_cases.SCRUB_ENV + ("NBX_WIDE_ACCUM",)}
    env.update(clique_cases.CHILD_ENV)
    proc = subprocess.run([sys.executable, WORKER, mode, str(out_file)], capture_output=True, text=True, timeout=LIMIT,
                          cwd=ROOT, env=env)
    res = None
    if out_file.exists():
        with open(out_file, "rb") as f:
            res = pickle.load(f)
    if res is not None and "async_error" in res:
        pytest.fail(f"a device wait gave up: {res['async_error']}\n{proc.stderr[-1500:]}")
    assert proc.returncode == 0 and res is not None, f"worker exit {proc.returncode}:\n{proc.stderr[-3000:]}"
    return res


def _check(oracle, res, name, want_record):
    failures = []
    for i, (kind, dt, op) in enumerate(ww.clique_cases()):
        xs = ww.inputs(oracle, kind, dt, op)
        exp = cases.expected_with(cases.wide_fold_of, oracle, xs, kind, dt, op, ww.N, ww.ROOT_RANK, ww.COUNT)
        bufs, recs = res[(name, i)]
        ctx = f"{name} {kind} {oracle.TYPE_NAMES[dt]} wide op {op}"
        bad = want_record([tuple(x) for x in recs])
        if bad:
            failures.append(f"{ctx}: launch records {recs}: {bad}")
        for r in range(ww.N):
            if r not in exp:
                assert bufs[r] is None
                continue
            e = np.ascontiguousarray(exp[r])
            buf = bufs[r]
            if not ((buf[:GUARD] == 0xA5).all() and (buf[GUARD + e.nbytes:] == 0xA5).all()):
                failures.append(f"{ctx} rank {r}: guard bytes overwritten")
            try:
                mi.assert_same(buf[GUARD:GUARD + e.nbytes].copy().view(oracle.NP_STORAGE[dt]), e, dt)
            except AssertionError as err:
                failures.append(f"{ctx} rank {r}: {err}")
    assert not failures, f"{len(failures)} failure(s):\n" + "\n".join(failures[:8])


def test_clique_fold_path(oracle, tmp_path):
    """Ranks sharing a GPU, the default: one record per rank's fold, of the wide core (6 packs,
    7 elements), source-type output (bit 1 clear), 3 sources."""
    def want(recs):
        if len(recs) != ww.N:
            return f"expected {ww.N} records"
        if any(f not in (cases.FAM_WIDE_PACKS, cases.FAM_WIDE_ELTS) or ns != ww.N or fl & 2 for f, ns, u, fl in recs):
            return "expected the wide core's families 6 / 7 with 3 sources"
        return None
    _check(oracle, _run(tmp_path, "fold"), "fold", want)


def test_clique_in_kernel(oracle, tmp_path):
    """NBX_CLIQUE_LL=1: the multi-process kernels' wide instantiation, one record per rank."""
    res = _run(tmp_path, "kernel")
    _check(oracle, res, "ll", lambda recs: None if recs == [(8, ww.N, 1, cases.FLAG_WIDE)] * ww.N else "expected LL, wide")
    _check(oracle, res, "simple",
           lambda recs: None if recs == [(11, ww.N, 0, cases.FLAG_WIDE)] * ww.N else "expected Simple direct, wide")


def test_one_rank(oracle, tmp_path):
    res = _run(tmp_path, "onerank")
    assert res["bad"] == [4, 4, 4, 4, 4, -7]
    user, second, again, unknown = res["slots"]
    assert user >= 5 and second >= 5 and second != user     # user handles lie past the built-in ops
    assert again == user                                     # the freed slot is the next one handed out
    assert unknown == 4
    assert res["mismatch"] == 4                              # a bf16 call with an f16 handle
    x, out_of_place, in_place, recs = res["copy"]
    assert np.array_equal(out_of_place, x) and np.array_equal(in_place, x)
    assert recs == [] and res["async"] == 0                  # a copy: never the PreMulSum kernel
