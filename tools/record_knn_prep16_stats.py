"""Record knn_stats() of every case of tests/test_knn_prep16_gpu.py with the library PM_LIB_PATH names (default: the tree's).

    PM_LIB_PATH=<parent build>/libpm_hip.so python tools/record_knn_prep16_stats.py out.json

tests/golden/knn_prep16_stats.json is such a record of the commit before the L2 matcher's kernels were filed by stage.
Results are also compared with the oracle, so a record is only written for a library that is right."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import points_matching_amd as pm  # noqa: E402
import test_knn_prep16_gpu as T  # noqa: E402
from oracle import pm_oracle as O  # noqa: E402


def main(out):
    O.build()
    rec = {}

    def one(ctx, cid, q, t, k, flags, misaligned=False, seeded=False):
        got, st = T.knn_dev(ctx, q, t, k, flags, misaligned, seeded)
        want = O.bf_knn_l2(q, t, k, nthreads=8)
        ok = (got["trainIdx"] == want["trainIdx"]).all() and (got["distance"].view(np.uint32) == want["distance"].view(np.uint32)).all()
        assert ok, cid
        assert cid not in rec, cid
        rec[cid] = st

    with pm.Context(0) as ctx:
        for nq, nt in T.SHAPES:
            for dim in T.DIMS:
                for i, kind in enumerate(T.KINDS):
                    q, t, flags = T.make(kind, nq, nt, dim, 100000 * nq + 100 * nt + dim + 7 * i)
                    one(ctx, T.shape_id(kind, nq, nt, dim), q, t, 2, flags)
        for case in T.edge_cases():
            one(ctx, *case)
    with open(out, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded", len(rec), "cases with", pm.api.LIB_PATH)


if __name__ == "__main__":
    main(sys.argv[1])
