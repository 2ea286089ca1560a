"""CPU: the pair list of tests/pairs_cases.py through the float64 restatements, two ways each (gn_cases.reference's rule).
It is the proof that the comparison of the pair-list entries against the restatements (tests/test_pairs_gpu.py) leaves out
one named pair and no other, and that the list ends its jobs every way a job can end."""
import pytest

import pairs_cases as PC


@pytest.mark.parametrize("method", PC.METHODS)
def test_the_restatements_call_every_pair_but_the_named_one_stable(oracle_mod, method):
    """Under both blocks.  The cap on what may be left out: (a2_n6, a0) for point-to-plane, nothing else."""
    assert PC.LEFT_OUT == {("p2l", "a2_n6", "a0")}
    unstable = set()
    for block in PC.BLOCKS:
        for p in PC.pairs(block):
            r = PC.reference(p, method, block, oracle_mod)
            print(f"{method} {block} ({p['src']}, {p['tgt']}): {'stable' if r['stable'] else 'UNSTABLE'}, iters {r['ref']['iters']}, "
                  f"status {r['ref']['status']}, floor {r['floor'][0]:.1e} m {r['floor'][1]:.1e} rad")
            if not r["stable"]:
                unstable.add((method, p["src"], p["tgt"]))
    assert unstable <= PC.LEFT_OUT, unstable
    if method == "p2l":
        assert unstable == PC.LEFT_OUT              # (the restatement does part there: the pair is left out for a reason)


@pytest.mark.parametrize("method", PC.METHODS)
def test_the_list_ends_every_way(oracle_mod, method):
    """P1: jobs at the cap, converged at different passes, degenerate at once -- exactly the named ones.  P2: every job that
    is not degenerate at once runs its 4 passes, but for the left-out pair, which loses its system on the way."""
    assert len(PC.pairs("P1")) == 22 and len(PC.pairs("P2")) == 21
    ends = {}
    for block in PC.BLOCKS:
        for p in PC.pairs(block):
            ref = PC.reference(p, method, block, oracle_mod)["ref"]
            key = "far" if PC.is_far(p) else (p["src"], p["tgt"])
            at_once = ref["status"] == 2 and ref["iters"] == 0
            assert at_once == (key in PC.DEGENERATE[method]), (method, block, key, ref["iters"], ref["status"])
            if (method, p["src"], p["tgt"]) in PC.LEFT_OUT:
                continue
            ends.setdefault(block, []).append((ref["status"], ref["iters"]))
            if block == "P2" and not at_once:
                assert (ref["status"], ref["iters"]) == (0, 4), (method, key)
    p1 = ends["P1"]
    converged_at = {i for s, i in p1 if s == 1}
    assert (0, 6) in p1 and len(converged_at) >= 3 and converged_at <= set(range(1, 7)) and (2, 0) in p1, p1
