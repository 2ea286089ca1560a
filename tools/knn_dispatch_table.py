"""Which launches a descriptor kNN search makes: for the smallest shape that reaches each branch of the search's plan
(csrc/knn_plan.hpp), the launch count of every profile family and the plan as stats() reports it.  A change of the
host side of the search that is meant to leave the launch sequences alone prints the same table before and after
(profiles/knn_dispatch_table.txt)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gloc3d_amd import capi, synth  # noqa: E402

FAMILIES = ("split_queries", "dist_mfma", "dist_exact", "select", "select_rerank", "rerank", "finalize")
STATS = ("last_n_tile", "last_k_split", "last_candidates", "queries_fallback")
# (branch reached, rows, dim, queries, k, algo, first row, clustered rows)
SHAPES = [
    ("fused, small window, split-bf16", 3000, 256, 24, 20, 2, 0, False),
    ("64 candidates, not fused", 3000, 256, 24, 52, 2, 0, False),
    ("large window, block minima, one K-split", 40001, 64, 9, 20, 2, 13, False),
    ("large window, slices, two K-splits, one redo launch", 20000, 256, 9, 20, 2, 0, True),
    ("large window, 64 candidates, flagged exact pass", 17000, 64, 12, 52, 2, 0, False),
    ("more than 768 work-groups, queries split ahead", 100000, 64, 9, 20, 2, 0, False),
    ("dim % 8 != 0: fp32 tiles under algo 2", 3000, 100, 24, 20, 2, 0, False),
    ("dim > 4096, not fused", 300, 4104, 9, 20, 2, 0, False),
    ("fp32 tiles, WQ = 1", 3000, 256, 9, 20, 3, 0, False),
    ("fp32 tiles, WQ = 2", 3000, 256, 24, 20, 3, 0, False),
    ("fp32 tiles, WQ = 4", 3000, 256, 70, 20, 3, 0, False),
    ("the 32 x 32 tiles", 98304, 64, 33, 20, 3, 0, False),
    ("exact, one-query streaming kernel", 4541, 4096, 1, 20, 1, 0, False),
    ("exact, general kernel", 4541, 4096, 9, 20, 1, 0, False),
    ("exact, k > 64: chunks and merge", 20000, 64, 3, 100, 1, 0, False),
]


def main():
    print(f"{'branch reached':52s} {'rows':>6s} {'dim':>4s} {'q':>3s} {'k':>3s} a {'first':>5s} | "
          + " ".join(f"{f:>13s}" for f in FAMILIES) + " | " + " ".join(f"{s:>16s}" for s in STATS))
    for i, (name, rows, dim, nq, k, algo, first, clustered) in enumerate(SHAPES):
        ix = capi.KnnIndex(dim)
        ix.set_option(capi.KNN_OPT_ALGO, algo)
        if clustered:  # as test_unproven_queries_above_16384_rows_are_redone_on_the_device builds them
            base = synth.descriptors_iid(71, 0, 1, dim)
            ix.add((base + np.float32(2e-4) * synth.descriptors_iid(72, 0, first + rows, dim)).astype(np.float32))
            q = (base + np.float32(2e-4) * synth.descriptors_iid(73, 0, nq, dim)).astype(np.float32)
        else:
            ix.add_synthetic(0, 1000 + i, 0, first + rows)
            q = synth.descriptors_iid(2000 + i, 0, nq, dim)
        ix.set_option(capi.KNN_OPT_PROFILE, 1)
        ix.search(q, k, first_row=first)
        counts = [ix.profile(f)[1] for f in FAMILIES]
        st = ix.stats()
        print(f"{name:52s} {rows:6d} {dim:4d} {nq:3d} {k:3d} {algo} {first:5d} | "
              + " ".join(f"{c:13d}" for c in counts) + " | " + " ".join(f"{st[s]:16d}" for s in STATS), flush=True)
        ix.close()


if __name__ == "__main__":
    main()
