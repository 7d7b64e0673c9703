"""GPU parity at the BASELINE shapes against fixtures generated from the REAL reference
(tests/golden/g8_large.json, tools/gen_golden_large.py): nothing is sampled or shrunk.

  cfg 3   256 LPs per family at 32 x 64 through the LDS-resident batch kernel: status, objective bits,
          solution CRC of every LP (SURVEY 8c G3 as specified)
  cfg 4   exact rational simplex, tableau 1024 x 2048, K = 8 and 16: whole-tableau checksums, objective row,
          basis; and the same solve bit for bit against the oracle
  cfg 2b  LP m = 4096, n = 8192 (slack tableau 4096 x 12289), K = 16 / 32 / 48: whole-tableau checksums,
          objective row, basis (SURVEY 8d cfg 2b)
Checksums: CRC-32 of the raw bytes, wrapping uint64 sum and xor of the words -- a checksum of checksums."""
import json
import os
import zlib

import numpy as np
import pytest

from conftest import needs_hooks

from tools import gen

pytestmark = pytest.mark.gpu
F64, RAT = 0, 1
GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g8_large.json")))


def checksum(a):
    a = np.ascontiguousarray(a)
    v = a.view(np.uint64).reshape(-1) if a.dtype.itemsize == 8 else a.view(np.uint32).reshape(-1).astype(np.uint64)
    return dict(crc32="%08x" % (zlib.crc32(a.tobytes()) & 0xFFFFFFFF), sum="%016x" % int(v.sum(dtype=np.uint64)),
                xor="%016x" % int(np.bitwise_xor.reduce(v)))


@pytest.mark.parametrize("fam", [0, 1])
def test_cfg3_batch_256_lps_per_family_against_the_reference(ctx, fam):
    rec = GOLD["g3_large"][fam]
    assert rec["family"] == fam
    leq, tg = gen.small_lp_batch_f64(256, 32, 64, fam, seed=gen.XS_SEED + rec["seed_offset"])
    status, v, sol = ctx.six_batch(F64, True, tg, leq)
    seen = set()
    for b, want in enumerate(rec["records"]):
        assert status[b] == want["status"], (fam, b, status[b], want["status"])
        assert float(v[b]).hex() == want["v"], (fam, b)
        if want["status"] == 0:
            assert "%08x" % (zlib.crc32(np.ascontiguousarray(sol[b]).tobytes()) & 0xFFFFFFFF) == want["sol_crc32"], (fam, b)
        seen.add(want["status"])
    assert len(seen) >= 2


@pytest.mark.parametrize("idx", [0, 1])
def test_cfg4_rational_1024x2048_against_the_reference(ctx, idx):
    import xpoly_amd
    rec = GOLD["g4_large"][idx]
    leq, tgtf = gen.int_lp_rat(1024, 1023)
    six = xpoly_amd.SIX(ctx, RAT)
    six.set_param(0, rec["K"])
    got = six.TwoStageMethod(leq, tgtf)
    assert got["status"] == rec["status"] and got["rhs"] == rec["rhs"]
    assert got["tab"].shape[:2] == (1024, 2048)
    assert checksum(got["tab"]) == rec["tab"]
    assert checksum(got["tgtf"]) == rec["tgtf"]
    assert got["tgtf"][got["rhs"]].tolist() == rec["obj_const"]
    assert checksum(got["eq2bv"].astype(np.int32)) == rec["eq2bv"]
    assert got["eq2bv"][:32].tolist() == rec["eq2bv_head"]
    assert rec["appro_calls"] > 100000 or rec["K"] < 16      # the fixture crosses the float32 rescue en masse


def test_cfg4_rational_1024x2048_k16_matches_oracle_bit_for_bit(ctx, port):
    import xpoly_amd
    leq, tgtf = gen.int_lp_rat(1024, 1023)
    want = port.two_stage(RAT, leq, tgtf, 16)
    six = xpoly_amd.SIX(ctx, RAT)
    six.set_param(0, 16)
    got = six.TwoStageMethod(leq, tgtf)
    assert got["status"] == want["status"] == 4
    for k in ("tab", "tgtf", "nvset", "bvset", "bv2eq", "eq2bv"):
        assert np.array_equal(got[k], want[k]), k


def test_cfg2b_lp_4096x8192_against_the_reference(ctx):
    """The end-to-end LP of BASELINE configs[1]: m = 4096, n = 8192, slack tableau 4096 x 12289. After 16, 32
    and 48 pivots the whole tableau (403 MB), the objective row and the basis are the reference's."""
    import xpoly_amd
    leq, tgtf = gen.dense_lp_f64(4096, 8192)
    lp = xpoly_amd.DeviceLP(ctx, F64, leq, tgtf)
    lp.begin()
    done = 0
    for rec in GOLD["g2_large"]:
        assert lp.iterate(rec["K"] - done) == xpoly_amd.six.XPG_RUNNING
        done = rec["K"]
        got = lp.read()
        assert list(got["tab"].shape) == rec["tab_shape"] and got["rhs"] == rec["rhs"]
        assert checksum(got["tab"]) == rec["tab"], rec["K"]
        assert checksum(got["tgtf"]) == rec["tgtf"], rec["K"]
        assert float(got["tgtf"][got["rhs"]]).hex() == rec["obj_const"]
        assert checksum(got["eq2bv"].astype(np.int32)) == rec["eq2bv"]
        assert sorted(int(x) for x in got["eq2bv"] if x < 8192) == rec["entered"]
        del got
    lp.close()


GOLD_BENCH = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_bench_lp.json")))


def check_bench_lp_state(got, rec):
    """One record of tests/golden/g11_bench_lp.json (tools/gen_golden_bench.py: the REAL reference's
    SIX::TwoStageMethod with set_param(0, K) on the bench LP) against a downloaded device state."""
    assert list(got["tab"].shape) == rec["tab_shape"] and got["rhs"] == rec["rhs"]
    assert checksum(got["eq2bv"].astype(np.int32)) == rec["eq2bv"], rec["K"]
    assert [int(x) for x in got["eq2bv"][:32]] == rec["eq2bv_head"], rec["K"]
    assert checksum(got["bv2eq"].astype(np.int32)) == rec["bv2eq"], rec["K"]
    assert float(got["tgtf"][got["rhs"]]).hex() == rec["obj_const"], rec["K"]
    assert checksum(got["tgtf"]) == rec["tgtf"], rec["K"]
    assert checksum(got["tab"]) == rec["tab"], rec["K"]


def test_bench_lp_through_the_whole_timed_range_against_the_reference(ctx):
    """The exact LP bench.py times (gen.hard_lp_f64(4096, 4095), slack tableau 4096 x 8192), through the default
    device loop (blocked + chain) to K = 1024, 2048 and 3840 pivots -- 3840 is where a bench step ends -- with the
    whole 268 MB tableau, the objective row and the basis compared with what the reference left there
    (src/com/lpsol.h:1039-1188 through :1907-1930)."""
    import xpoly_amd
    leq, tgtf = gen.hard_lp_f64(4096, 4095)
    lp = xpoly_amd.DeviceLP(ctx, F64, leq, tgtf)
    lp.begin()
    done = 0
    for rec in GOLD_BENCH["bench_lp"]:
        assert rec["status"] == 4                      # SIX_TIME_OUT: the reference stopped at max_iter = K
        assert lp.iterate(rec["K"] - done) == xpoly_amd.six.XPG_RUNNING
        done = rec["K"]
        assert lp.pivots_done() == done
        got = lp.read()
        check_bench_lp_state(got, rec)
        del got
    # and a second solve on the same handle, straight to the end of a bench step, as the timed loop does it
    lp.begin()
    assert lp.iterate(3840) == xpoly_amd.six.XPG_RUNNING
    check_bench_lp_state(lp.read(), GOLD_BENCH["bench_lp"][-1])
    lp.close()


def test_bench_plain_run_dumps_the_state_of_its_last_step(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR`: the plain run prints one JSON line with the contract's
    keys and nothing of --full, and DIR holds float64 arrays of the state its last timed step left -- basis maps and
    objective row equal to the reference's TwoStageMethod(max_iter = 3840) on the bench LP, under 64 MB in all."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=root)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["steps"] == 2 and out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "pivots/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f64" and out["config"]["tableau"] == [4096, 8192]
    assert not {"batched", "cfg2b", "self_check", "cpu_baseline", "roofline"} & set(out)
    arrays = {n: np.load(os.path.join(str(tmp_path), n + ".npy")) for n in out["outputs"]["arrays"]}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    rec = GOLD_BENCH["bench_lp"][-1]
    assert rec["K"] == 3840
    assert checksum(arrays["eq2bv"].astype(np.int32)) == rec["eq2bv"] and checksum(arrays["bv2eq"].astype(np.int32)) == rec["bv2eq"]
    assert checksum(arrays["objective_row"]) == rec["tgtf"]
    assert arrays["tableau_rows"].shape == (512, 8192) and arrays["tableau_rhs_column"].shape == (4096,)
    assert np.isin(arrays["tableau_rows"][:, -1], arrays["tableau_rhs_column"]).all()      # sampled rows of the same tableau


@needs_hooks
def test_chain_roll_call_abort_falls_back_bit_exactly(monkeypatch):
    """ADVICE / VERDICT round 2 item 8: the persistent chain launch needs all its workers resident at once. A launch whose
    roll call fails (here forced on every 3rd batch by the test hook) leaves without touching the state: the batch
    closes with stage 0's pivot, the sweep applies it, and the host -- once it has seen the abort at a status read --
    enqueues launch-per-stage kernels for the rest of the solve. The state after 1024 pivots is the reference's."""
    import xpoly_amd
    monkeypatch.setenv("XPG_CHAIN_TEST_ABORT", "3")
    c = xpoly_amd.Context(0)
    leq, tgtf = gen.hard_lp_f64(4096, 4095)
    lp = xpoly_amd.DeviceLP(c, F64, leq, tgtf)
    lp.begin()
    rec = GOLD_BENCH["bench_lp"][0]
    done = 0
    while done < rec["K"]:                               # aborted batches stage one pivot instead of 16: iterate until there
        assert lp.iterate(rec["K"] - done) == xpoly_amd.six.XPG_RUNNING
        done = lp.pivots_done()
    aborts, off = lp.chain_aborts()
    assert aborts >= 1 and off                           # the first call aborted some launches, then the handle switched over
    check_bench_lp_state(lp.read(), rec)
    lp.begin()                                           # a new solve re-arms the chain
    assert lp.chain_aborts() == (0, False)
    lp.close(); c.close()


@needs_hooks
def test_chain_placement_check_failure_switches_to_the_spread_form(monkeypatch):
    """Round 4: the chain's workers are the workgroups with blockIdx % 8 == 0, which the dispatcher puts on ONE XCD -- an
    observation, not a contract, so the roll call checks it (a counter per XCD id). The test hook makes every second
    one-XCD launch "find" its workers on several XCDs: that launch aborts without touching the state, the host switches the
    solve to the spread form of the kernel (sc1 stores, any placement) -- NOT to launch-per-stage kernels -- and the state
    after 1024 pivots is the reference's. Most batches still have their first stage inside the chain launch."""
    import xpoly_amd
    monkeypatch.setenv("XPG_CHAIN_TEST_ABORT", "-2")
    c = xpoly_amd.Context(0)
    leq, tgtf = gen.hard_lp_f64(4096, 4095)
    lp = xpoly_amd.DeviceLP(c, F64, leq, tgtf)
    lp.begin()
    rec = GOLD_BENCH["bench_lp"][0]
    assert lp.iterate(rec["K"]) == xpoly_amd.six.XPG_RUNNING      # (iterate re-queues what an aborted batch left undone)
    assert lp.pivots_done() == rec["K"]
    aborts, off = lp.chain_aborts()
    assert aborts >= 1 and not off                       # placement failures are counted as aborts, the chain stays on
    assert lp.chain_runs >= 20 and lp.chain_folds() >= 10
    check_bench_lp_state(lp.read(), rec)
    lp.close(); c.close()


@needs_hooks
def test_chain_folds_stage_zero_and_the_unfolded_loop_agree(monkeypatch):
    """Round 4: in the steady state a batch is [chain launch incl. stage 0, sweep]; XPG_CHAIN_FOLD=0 keeps stage 0 as
    launches of its own. Same state either way (= the reference's at K = 1024), and the folded run really folded."""
    import xpoly_amd
    rec = GOLD_BENCH["bench_lp"][0]
    leq, tgtf = gen.hard_lp_f64(4096, 4095)
    folds = {}
    for fold in ("1", "0"):
        monkeypatch.setenv("XPG_CHAIN_FOLD", fold)
        c = xpoly_amd.Context(0)
        lp = xpoly_amd.DeviceLP(c, F64, leq, tgtf)
        lp.begin()
        for k in (100, rec["K"] - 100):                  # two calls: each starts with stage-0 launches
            assert lp.iterate(k) == xpoly_amd.six.XPG_RUNNING
        assert lp.pivots_done() == rec["K"]
        folds[fold] = lp.chain_folds()
        check_bench_lp_state(lp.read(), rec)
        lp.close(); c.close()
    assert folds["0"] == 0 and folds["1"] >= rec["K"] // 32 - 4            # (32 pivots per batch, the default)


BUSY_SCRIPT = r"""
import json, os, sys, zlib
import numpy as np
import torch                                   # torch's HIP runtime first, then the library's (the order bench.py uses)
torch.zeros(1, device="cuda")
sys.path.insert(0, sys.argv[1])
import xpoly_amd
from tools import gen
ctx = xpoly_amd.Context(0)
leq, tgtf = gen.hard_lp_f64(4096, 4095)
lp = xpoly_amd.DeviceLP(ctx, 0, leq, tgtf)
side = torch.cuda.Stream()
a = torch.randn(8192, 8192, device="cuda"); b = torch.randn(8192, 8192, device="cuda")
lp.begin()
K, done = int(sys.argv[2]), 0
while done < K:
    with torch.cuda.stream(side):
        for _ in range(24):                    # back-to-back 8192^3 fp32 GEMMs on every CU while the LP iterates
            a = (a @ b) * 1e-2
    assert lp.iterate(min(256, K - done)) == xpoly_amd.six.XPG_RUNNING
    done = lp.pivots_done()
torch.cuda.synchronize()
got = lp.read()
def checksum(x):
    x = np.ascontiguousarray(x)
    v = x.view(np.uint64).reshape(-1) if x.dtype.itemsize == 8 else x.view(np.uint32).reshape(-1).astype(np.uint64)
    return dict(crc32="%08x" % (zlib.crc32(x.tobytes()) & 0xFFFFFFFF), sum="%016x" % int(v.sum(dtype=np.uint64)), xor="%016x" % int(np.bitwise_xor.reduce(v)))
print(json.dumps(dict(tab=checksum(got["tab"]), tgtf=checksum(got["tgtf"]), eq2bv=checksum(got["eq2bv"].astype(np.int32)),
                      aborts=lp.chain_aborts()[0], chain_off=lp.chain_aborts()[1])))
"""


def test_chain_under_a_busy_device_stays_bit_exact():
    """The same LP while another stream of the process keeps every CU busy with large GEMMs (a host application's own
    work): whatever mix of completed chains, aborted roll calls and launch-per-stage batches results, the state after
    1024 pivots is the reference's. In a process of its own: torch's HIP runtime has to come up before the library's."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = GOLD_BENCH["bench_lp"][0]
    r = subprocess.run([sys.executable, "-c", BUSY_SCRIPT, root, str(rec["K"])], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print("chain under a busy device: roll calls failed %d, switched to launch-per-stage: %s" % (out["aborts"], out["chain_off"]))
    assert out["tab"] == rec["tab"] and out["tgtf"] == rec["tgtf"] and out["eq2bv"] == rec["eq2bv"]


def test_cfg2b_bench_lp_against_the_reference(ctx):
    """The LP bench.py's cfg2b leg times -- gen.hard_lp_f64(4096, 8192), slack tableau 4096 x 12289 (403 MB, ld 12352) --
    after the 256 + 1024 pivots of one pass: whole tableau, objective row and basis are what the real reference's
    TwoStageMethod(max_iter = 1280) leaves (tests/golden/g11_bench_lp.json cfg2b_lp, tools/gen_golden_bench.py cfg2b)."""
    import xpoly_amd
    recs = GOLD_BENCH.get("cfg2b_lp", [])
    assert recs, "fixture missing: run tools/gen_golden_bench.py cfg2b in the authoring container"
    rec = recs[0]
    leq, tgtf = gen.hard_lp_f64(4096, 8192)
    lp = xpoly_amd.DeviceLP(ctx, F64, leq, tgtf)
    del leq
    lp.begin()
    assert lp.iterate(256) == xpoly_amd.six.XPG_RUNNING
    assert lp.iterate(rec["K"] - 256) == xpoly_amd.six.XPG_RUNNING
    assert lp.pivots_done() == rec["K"]
    check_bench_lp_state(lp.read(), rec)
    lp.close()


def signed_lp_rat(m, n, seed):
    """Signed integer data with repeated ratios (ties, relaxed ratio passes, disabled columns) and a feasible origin."""
    rng = np.random.default_rng(seed)
    A = rng.integers(-3, 7, size=(m, n)).astype(np.int32)
    A[rng.random((m, n)) < 0.5] = 0
    b = (rng.integers(1, 4, size=m) * 6).astype(np.int32)
    c = rng.integers(-2, 5, size=n).astype(np.int32)
    return gen.to_rat(np.concatenate([A, b[:, None]], axis=1)), gen.to_rat(np.concatenate([c, [0]]).astype(np.int32))


@pytest.mark.parametrize("m,n,seed", [(300, 200, 1), (520, 130, 2), (700, 90, 3), (257, 600, 4)])
def test_rational_pipelined_loop_with_several_pick_workgroups(ctx, port, m, n, seed):
    """The pipelined rational loop on tableaux of more than 256 rows: the sweep launch carries 2-3 pick workgroups
    whose records the last adder combines (lp_pipe_r32.hip.h). States after 1, 7, 33 pivots and at the end (optimum
    or 100 iterations) against the oracle, dense positive data and signed data with ties and deferred branches."""
    import xpoly_amd
    six = xpoly_amd.SIX(ctx, RAT)
    for fam in (0, 1):
        leq, tg = gen.int_lp_rat(m, n, seed=gen.XS_SEED + seed) if fam == 0 else signed_lp_rat(m, n, seed)
        for K in (1, 7, 33, 100):
            want = port.two_stage(RAT, leq, tg, K)
            six.set_param(0, K)
            got = six.TwoStageMethod(leq, tg)
            assert got["status"] == want["status"], (fam, K, got["status"], want["status"])
            for k in ("tab", "tgtf", "nvset", "bvset", "bv2eq", "eq2bv"):
                assert np.array_equal(got[k], want[k]), (fam, K, k)
            if want["status"] == 0:
                assert np.array_equal(got["maxv"], want["maxv"]) and np.array_equal(got["sol"], want["sol"])


PIPE_R32_SCRIPT = r"""
import json, sys, zlib
import numpy as np
sys.path.insert(0, sys.argv[1])
import xpoly_amd
from tools import gen
ctx = xpoly_amd.Context(0)
leq, tgtf = gen.int_lp_rat(1024, 1023)
six = xpoly_amd.SIX(ctx, 1)
six.set_param(0, 16)
got = six.TwoStageMethod(leq, tgtf)
def checksum(x):
    x = np.ascontiguousarray(x)
    v = x.view(np.uint64).reshape(-1) if x.dtype.itemsize == 8 else x.view(np.uint32).reshape(-1).astype(np.uint64)
    return dict(crc32="%08x" % (zlib.crc32(x.tobytes()) & 0xFFFFFFFF), sum="%016x" % int(v.sum(dtype=np.uint64)), xor="%016x" % int(np.bitwise_xor.reduce(v)))
print(json.dumps(dict(tab=checksum(got["tab"]), tgtf=checksum(got["tgtf"]), eq2bv=checksum(got["eq2bv"].astype(np.int32)))))
"""


def test_cfg4_rational_two_launch_loop_against_the_reference():
    """XPG_R32_LOOP=pipe (the two-launch prep -> sweep loop; the fused one-launch loop is the default at this size) reaches
    the same state as the real reference on the 1024 x 2048 LP after 16 pivots. The switch is read once per process, hence
    a process of its own."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    rec = [r for r in GOLD["g4_large"] if r["K"] == 16][0]
    env = dict(os.environ, XPG_R32_LOOP="pipe")
    r = subprocess.run([sys.executable, "-c", PIPE_R32_SCRIPT, root], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["tab"] == rec["tab"] and out["tgtf"] == rec["tgtf"] and out["eq2bv"] == rec["eq2bv"]
