"""The oracle side of tests/test_gpu_per_rng.py, without a GPU: the predicted device-RNG draws of the chunk replay's
samplers (oracle.rng per_stratum_fracs / per_uniform_slots) are well-formed, and every case the GPU test compares
exactly keeps its draws clear of the node boundaries (per_rng_cases.descent_margin >= MARGIN_MIN)."""
import numpy as np
import pytest

import per_rng_cases as pc
from oracle import rng as orng

COUNTERS = [pc.COUNTER + i for i in range(pc.CALLS)]
ALL_CASES = pc.CASES + pc.PACK_CASES


def test_fracs_in_unit_interval_and_distinct():
    fr = [orng.per_stratum_fracs(pc.SEED, c, 8192) for c in COUNTERS]
    for f in fr:
        assert f.dtype == np.float64 and f.min() >= 0.0 and f.max() < 1.0
        assert len(np.unique(f)) == f.size                  # 53-bit draws: no two k share a fraction
        assert 0.45 < f.mean() < 0.55
    for a, b in zip(fr, fr[1:]):
        assert not np.array_equal(a, b)                     # a fresh stream per counter
        assert not np.array_equal(a[1:], b[:-1])            # and not the same stream shifted by one
    # a prefix of a longer call's draws: draw k does not depend on B
    np.testing.assert_array_equal(orng.per_stratum_fracs(pc.SEED, 5, 33), fr[0][:33])
    # the two samplers' streams differ, and the seed matters
    assert not np.array_equal(orng._unit53(pc.SEED, 5, 64, orng.PER_TAG_UNIFORM), fr[0][:64])
    assert not np.array_equal(orng.per_stratum_fracs(pc.SEED + 1, 5, 64), fr[0][:64])


def test_fracs_restate_rng_draw():
    """One value by hand: the top 53 bits of rng_draw(seed, ctr, k, 77), scaled by 2^-53."""
    r = int(orng.rng_draw(np.uint64(1234), np.uint64(6), np.uint64(40), np.uint64(77)))
    assert orng.per_stratum_fracs(1234, 6, 41)[40] == (r >> 11) / 2.0 ** 53
    r = int(orng.rng_draw(np.uint64(1234), np.uint64(6), np.uint64(40), np.uint64(91)))
    assert orng.per_uniform_slots(1234, 6, 41, 2500)[40] == min(2499, int((r >> 11) / 2.0 ** 53 * 2500))


@pytest.mark.parametrize("n", [1, 5, 2500])
def test_uniform_slots_in_range(n):
    seen = []
    for c in (3, 4):
        sl = orng.per_uniform_slots(77, c, 1000, n)
        assert sl.dtype == np.int64 and sl.min() >= 0 and sl.max() < n
        seen.append(sl)
    if n > 1:
        assert not np.array_equal(seen[0], seen[1])
        assert len(np.unique(seen[0][768:])) > 1
    if n == 5:
        assert set(seen[0].tolist()) == set(range(5))       # 1000 draws over 5 slots reach every slot


@pytest.mark.parametrize("seed", pc.SEEDS)
@pytest.mark.parametrize("flavor,cap,fill,B", ALL_CASES, ids=[f"{f}-{c}-{n}-{b}" for f, c, n, b in ALL_CASES])
def test_strata_and_margin(flavor, cap, fill, B, seed):
    ora = pc.filled_oracle(flavor, cap, fill)
    assert ora.n_data == fill
    prev = None
    for ctr in COUNTERS:
        fr = orng.per_stratum_fracs(seed, ctr, B)
        tree = ora.tree.copy()
        gap, nodes, s = pc._descend(tree, B, fr)
        seg = tree[0] / B
        k = np.arange(B)
        assert (s >= seg * k).all() and (s <= seg * (k + 1)).all()      # every s_k in its own stratum
        margin = pc.descent_margin(ora, B, fr)
        assert margin == gap / tree[0]
        print(f"{flavor} cap {cap} B {B} seed {seed} ctr {ctr}: margin {margin:.3e}")
        assert margin >= pc.MARGIN_MIN
        on, oslots, pri, w = pc.predict(ora, seed, ctr, B)               # anneals; vdn: decays the tree
        np.testing.assert_array_equal(on, nodes)                         # the vectorised descent is the oracle's
        np.testing.assert_array_equal(oslots, on - (cap - 1))
        assert oslots.min() >= 0 and oslots.max() < fill
        assert np.isfinite(w).all() and w.max() == 1.0 and w.min() > 0
        assert prev is None or not np.array_equal(on, prev)              # consecutive calls can be told apart
        prev = on
    assert abs(ora.beta - (pc.FLAVOR_KW[flavor]["beta"] + pc.CALLS * ora.beta_inc)) < 1e-12
