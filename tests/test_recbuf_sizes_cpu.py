"""CPU side of tests/test_gpu_recbuf_sizes.py: the case scripts of tests/recbuf_cases.py on the oracle alone.
What is asserted here is what the GPU comparison relies on: the sweep never samples an empty leaf (the weights
it compares are finite), the restated device draws are proper fractions, the big ring's update really carries a
duplicate across position 1024, and the first weights after a reference-mode insert are constant, so only the
second sample of each round can show the priorities."""
import functools

import numpy as np
import pytest

import recbuf_cases as rc


@functools.lru_cache(maxsize=None)
def big_ring_facts(leaf_mode):
    return rc.big_ring(leaf_mode, True)        # same_share moves bytes only: the facts do not depend on it


@pytest.mark.parametrize("size", rc.SWEEP_SIZES)
def test_sweep_fold_and_samples(size):
    rows = rc.length_sweep(size)
    lens = [r[0] for r in rows]
    assert lens == list(range(2, size + 1)) + [size] * rc.SWEEP_EXTRA_INSERTS
    for ln, idx, w, fold, fold_rec in rows:
        assert fold == fold_rec, (size, ln)
        assert idx.min() >= 0 and idx.max() < ln, (size, ln, idx)
        assert np.isfinite(w).all() and (w > 0).all(), (size, ln, w)
        assert idx[0] >= ln - 2, (size, ln, idx)                 # u = 1 - 2**-53 lands at the end of the mass
        if len(idx) > 1:
            assert idx[1] == 0, (size, ln, idx)                  # u = 0 lands on the first leaf


def test_sweep_reaches_the_fold_edges():
    """len - 2 takes the values itcap/2 - 1 (the fold ends on the left half's last leaf: itcap 4 .. 64) and
    itcap/2 (one leaf into the right half: itcap 4 .. 32), and itcap == size occurs (the root's range but one)."""
    ends = {(s, ln - 2) for s in rc.SWEEP_SIZES for ln in range(2, s + 1)}
    for itcap in (4, 8, 16, 32, 64):
        sizes = [s for s in rc.SWEEP_SIZES if itcap // 2 < s <= itcap]
        assert any((s, itcap // 2 - 1) in ends for s in sizes), itcap
        if itcap <= 32:
            assert any((s, itcap // 2) in ends for s in sizes), itcap
    assert {2, 4, 8, 16, 32} <= set(rc.SWEEP_SIZES)              # itcap == size
    assert len(set(rc.PRIO_TABLE.tolist())) == len(rc.PRIO_TABLE) and (rc.PRIO_TABLE > 0).all()


@pytest.mark.parametrize("kind", ["sum", "min"])
def test_one_set_call_equals_the_per_leaf_loop(kind):
    """RecBufferOracle.insert writes its leaves with one SegTree.set; the reference loops one per leaf."""
    from oracle.recbuf import SegTree
    rng = np.random.default_rng(4)
    a, b = SegTree(128, kind), SegTree(128, kind)
    start = rng.random(100) * 5 + 0.1
    a.set(np.arange(100), start)
    b.set(np.arange(100), start)
    leaves = (70 + np.arange(45)) % 100              # a wrapping slot range
    val = np.float32(2.5) ** 0.6
    for i in leaves:
        a.set(i, val)
    b.set(leaves, val)
    np.testing.assert_array_equal(a.v, b.v)


@pytest.mark.parametrize("leaf_mode", ["reference", "slots"])
def test_big_ring_facts(leaf_mode):
    c = rc.BIG
    f = big_ring_facts(leaf_mode)
    assert f["current"] == [0, 1500, 500]                        # the second insert wraps, the third starts mid-ring
    assert all(m > rc.GRID_SPAN for m in f["moved"])             # obs floats of one insert
    assert (c["T"] + 1) * c["B"] * c["N"] * c["D"] > rc.GRID_SPAN    # obs floats of one gather
    assert c["n_insert"] > 1024 and c["B"] > 1024
    for fr in f["fracs"]:
        assert fr.dtype == np.float64 and fr.min() >= 0.0 and fr.max() < 1.0
        assert len(np.unique(fr)) == c["B"]
    assert not np.array_equal(f["fracs"][0], f["fracs"][1])      # a fresh stream per call counter
    for idx in f["idx"]:
        assert rc.crosses(idx, 1024), "no duplicate pair across position 1024"
        assert len(np.unique(idx)) < c["B"]
    for w in f["first_w"] + f["second_w"]:
        assert np.isfinite(w).all()
    for w in f["second_w"]:
        assert w.min() < w.max()                                 # the updated priorities show
    if leaf_mode == "reference":
        for w in f["first_w"]:
            assert (w == 1.0).all()                              # the insert rewrote every leaf that carries mass
