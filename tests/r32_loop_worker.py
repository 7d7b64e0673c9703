"""Child process of tests/test_gpu_r32_loop_geometry.py: K-pivot prefixes and whole solves of the LPs of tests/r32_loop_cases.py
on the device-resident Rational loop the environment selects (XPG_R32_LOOP and XPG_R32_GENERIC_EVERY are read once per
process). R32_LOOP_CASES names the forced loop ("fused" / "pipe": the cases listed for it; empty: every case, the size rule
decides). One JSON line per (case, K): r32_loop_cases.record() of the result -- status, CRC-32 of every array of the state, the
pivot trace, for the exact set the columns the Fraction replay follows -- plus `ran`, the loop the handle's last iterations
took (xpg_lp_loop_info)."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import xpoly_amd                                        # noqa: E402
import r32_loop_cases as RC                             # noqa: E402

if __name__ == "__main__":
    env_loop = os.environ.get("R32_LOOP_CASES") or None
    ctx = xpoly_amd.Context()
    for case in RC.CASES:
        if not RC.runs_in(case, env_loop):
            continue
        leq, tg, _ = RC.build(case)
        for K in case["Ks"]:
            lp = xpoly_amd.DeviceLP(ctx, RC.RAT, leq, tg)
            st = lp.two_stage(K)
            res = lp.read()
            res["status"] = st
            res["trace"] = lp.trace()
            ran = lp.r32_loop_ran()
            lp.close()
            cols = RC.replay_cols(case["m"], case["nv"], res["trace"]) if case["exact"] else None
            rec = RC.record(res, case, K, cols)
            rec["ran"] = ran
            print(json.dumps(rec), flush=True)
    ctx.close()
