"""Child process of tests/test_gpu_batch_geometry.py: the SLICE_CASES of tests/batch_geometry.py through xpg_six_batch_* with
whatever XPG_BATCH_SLICE / XPG_BATCH_SLICE_FORCE the environment sets (read once per process, hooks build); one JSON line
per case with the status array, the value array's bytes and SHA-256 of the solutions of the LPs that ended with status 0."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import xpoly_amd                                        # noqa: E402
import batch_geometry as bg                             # noqa: E402

if __name__ == "__main__":
    ctx = xpoly_amd.Context()
    for cs in bg.SLICE_CASES:
        tg, lq = bg.caller_arrays(cs.kind, cs.is_max, bg.make_lps(cs))
        st, v, sol = ctx.six_batch(cs.kind, cs.is_max, tg, lq, max_iter=cs.limit)
        ok = st == 0
        solm = np.where(ok.reshape((-1,) + (1,) * (sol.ndim - 1)), sol, 0)      # (sol is left alone where the status is not 0)
        print(json.dumps(dict(id=bg.case_id(cs), status=st.tolist(), v=np.ascontiguousarray(v).tobytes().hex(),
                              sol=hashlib.sha256(np.ascontiguousarray(solm).tobytes()).hexdigest())), flush=True)
