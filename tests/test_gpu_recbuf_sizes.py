"""Device episode replay (csrc/recbuf.hip via minimarl.recbuf) against oracle.recbuf.RecBufferOracle and
oracle.rng at the sizes where each kernel loop takes its second pass. Scripts and comparison rules (exact
indices after the leaf sync, weights rtol 1e-6, everything else bit-exact): tests/recbuf_cases.py.

Which loop each test pushes past its first pass, and the count that proves it:

* test_big_ring: the copy kernels' grid-stride loop (grid capped at 2048 x 256 = 524,288 threads per field):
  an insert moves 4 x 1500 x 94 = 564,000 obs floats, a gather 4 x 1400 x 94 = 526,400 (1,052,800 of share_obs
  without same_share). erb_set_kernel (one block of 1024): 1500 leaves per insert and 1400 entries per update run
  its leaf-write, last-duplicate and ancestor loops twice, with duplicate indices on both sides of position
  1024. erb_sample_kernel (one block of 256): B = 1400 is six passes. The draws are the device RNG's, predicted.
* test_full_ring_one_insert: n == buffer_size = 1100 > 1024 from current = 300: every slot and every leaf is
  rewritten by one call (leaf loop: 1100 entries through the wrapping (base + i) % size path); then again from
  current == size, where the cursor stands after an insert that ends on the ring's last slot.
* test_update_second_pass: 1500 crafted entries into 2048 full leaves: every property (last duplicate wins, the
  maximum, the four kinds of rejected entry) sits at a position >= 1024, i.e. in the second pass only.
* test_length_sweep: no second pass, the prefix fold's path instead: len - 2 from 0 to 31 in trees of 2 .. 64
  leaves, both sides of every itcap / 2, itcap == size, and two inserts past the full ring (current == size).
* test_uniform_device_rng: erb_uniform_kernel with B = 1000 = 3 full blocks + 232 threads, at len 5 and 2500.
* test_insert_collected_second_pass: erb_insert_kernel<WRAP> (share_obs built from obs, r % Rw): one collect of
  E = 1400 moves 4 x 1400 x 94 = 526,400 floats of obs and of share_obs (1,052,800 without same_share).
"""
import numpy as np
import pytest
import torch

import recbuf_cases as rc
from oracle.recbuf import RecBufferOracle

pytestmark = pytest.mark.gpu
PID = rc.PID


@pytest.mark.parametrize("same_share", [True, False], ids=["same_share", "own_share"])
@pytest.mark.parametrize("leaf_mode", ["reference", "slots"])
def test_big_ring(leaf_mode, same_share):
    c = rc.BIG
    buf = rc.make(True, c["size"], c["T"], c["N"], c["D"], c["S"], c["A"], same_share, leaf_mode, seed=c["seed"],
                  alpha=c["alpha"])
    f = rc.big_ring(leaf_mode, same_share, buf)
    assert f["current"] == [0, 1500, 500] and all(m > rc.GRID_SPAN for m in f["moved"])
    for idx in f["idx"]:
        assert rc.crosses(idx, 1024)             # a duplicate pair with one entry in each pass of the update
    for w in f["second_w"]:
        assert w.min() < w.max()                 # the only sample of a reference-mode round that sees priorities


def test_full_ring_one_insert():
    SIZE, T, N, D, S, A = 1100, 2, 2, 3, 6, 3
    rng = np.random.default_rng(12)
    buf = rc.make(True, SIZE, T, N, D, S, A, True, "slots")
    ora = RecBufferOracle(SIZE, T, N, D, S, A, alpha=0.6, prioritized=True, leaf_mode="slots")
    first = rc.episodes(rng, 300, T, N, D, S, A)
    np.testing.assert_array_equal(buf.insert(300, *rc.as_dicts(first)), ora.insert(300, *first))
    # priorities on the first insert's leaves: the whole-ring insert has to replace them, not only fill zeros
    idx0 = np.arange(300)
    prio0 = (0.05 + 3.0 * rng.random(300)).astype(np.float32)
    buf.update_priorities(torch.as_tensor(idx0).cuda(), torch.as_tensor(prio0).cuda(), PID)
    ora.update_priorities(idx0, prio0)
    rc.sync_trees(buf, ora, "first insert")
    whole = rc.episodes(rng, SIZE, T, N, D, S, A)
    slots = buf.insert(SIZE, *rc.as_dicts(whole))
    np.testing.assert_array_equal(slots, (300 + np.arange(SIZE)) % SIZE)
    np.testing.assert_array_equal(slots, ora.insert(SIZE, *whole))
    assert len(buf) == len(ora) == SIZE
    allidx = np.arange(SIZE)
    rc.compare_batch(rc.gather_ring(buf, allidx), ora.sample_inds(allidx), "whole ring")
    np.testing.assert_array_equal(rc.gather_ring(buf, slots)[0][PID].cpu().numpy(), whole[0].transpose(2, 0, 1, 3))
    assert rc.sync_trees(buf, ora, "whole-ring insert") == 0
    # and the next insert starts where the oracle's does
    more = rc.episodes(rng, 7, T, N, D, S, A)
    np.testing.assert_array_equal(buf.insert(7, *rc.as_dicts(more)), ora.insert(7, *more))
    rc.compare_batch(rc.gather_ring(buf, allidx), ora.sample_inds(allidx), "after the next insert")
    # fill up to the ring's end (the cursor comes out equal to the size, not 0), then a whole ring from there
    for n, what in ((SIZE - 307, "to the end"), (SIZE, "whole ring from the end"), (5, "after it")):
        ep = rc.episodes(rng, n, T, N, D, S, A)
        want = ora.insert(n, *ep)
        np.testing.assert_array_equal(buf.insert(n, *rc.as_dicts(ep)), want, err_msg=what)
        rc.compare_batch(rc.gather_ring(buf, allidx), ora.sample_inds(allidx), what)
        assert rc.sync_trees(buf, ora, what) == 0
    np.testing.assert_array_equal(want, np.arange(5))
    buf.check_errors()


def test_update_second_pass():
    """The reference asserts on a bad entry; the kernel skips it and flags it. What the kernel does when a bad
    entry shares its index with a good one, or carries the largest priority, is not specified: the inputs avoid
    both."""
    SIZE, T, N, D, S, A = 2048, 1, 1, 1, 1, 2
    n = 1500
    rng = np.random.default_rng(31)
    buf = rc.make(True, SIZE, T, N, D, S, A, True, "slots")
    ora = RecBufferOracle(SIZE, T, N, D, S, A, alpha=0.6, prioritized=True, leaf_mode="slots")
    ep = rc.episodes(rng, SIZE, T, N, D, S, A)
    np.testing.assert_array_equal(buf.insert(SIZE, *rc.as_dicts(ep)), ora.insert(SIZE, *ep))
    rc.sync_trees(buf, ora, "insert")
    perm = rng.permutation(SIZE)
    idx = perm[:n].astype(np.int64)                       # distinct so far
    spare = perm[n:]                                      # indices no good entry names
    prio = (0.05 + 3.0 * rng.random(n)).astype(np.float32)       # all below 3.05
    # duplicates: across position 1024 (a pair and a triple), inside the first pass, inside the second
    idx[1300] = idx[10]
    idx[700] = idx[5]
    idx[1100] = idx[5]
    idx[900] = idx[20]
    idx[1450] = idx[1030]
    for late, early in ((1300, 10), (1100, 700), (700, 5), (900, 20), (1450, 1030)):
        assert idx[late] == idx[early] and prio[late] != prio[early]
    prio[1200] = np.float32(7.5)                          # the maximum, seen by a second-pass entry only
    bad = np.array([1050, 1051, 1052, 1053])
    idx[1050], idx[1051] = SIZE, -1                       # == len (the ring is full), negative
    idx[1052], idx[1053] = spare[0], spare[1]
    prio[1052], prio[1053] = np.float32(0.0), np.float32(np.nan)
    assert bad.min() >= 1024 and int(np.nanargmax(prio)) == 1200
    good = np.setdiff1d(np.arange(n), bad)
    assert not np.isin(idx[bad], idx[good]).any()
    before = buf.trees()
    buf.update_priorities(torch.as_tensor(idx).cuda(), torch.as_tensor(prio).cuda(), PID)
    ora.update_priorities(idx[good], prio[good])
    err = rc.sync_trees(buf, ora, "update")               # trees and max_priority == the oracle without the four
    assert err == 1 | 2, err                              # index flag and priority flag, not the gather's 4
    assert np.float32(buf.max_priority()) == np.float32(7.5)
    after = buf.trees()
    cap = ora.sum.cap
    # the leaves the two bad priorities name keep the insert's 1.0. The two bad indices name no leaf: len == itcap
    # lies past the tree, and -1 would be the internal node cap - 1, which sync_trees has compared bit for bit.
    for b, a in zip(before, after):
        for k in (spare[0], spare[1]):
            assert a[cap + k] == b[cap + k] == 1.0
    # the later duplicate won: the leaf holds the later priority ** alpha (one float32 ulp as in tree_close)
    for late in (1300, 1100, 900, 1450):
        want = np.float64(prio[late] ** np.float32(0.6))
        np.testing.assert_allclose(after[0][cap + idx[late]], want, rtol=rc.TREE_RTOL)
    with pytest.raises(AssertionError, match="index outside"):
        buf.check_errors()


@pytest.mark.parametrize("size", rc.SWEEP_SIZES)
def test_length_sweep(size):
    buf = rc.make(True, size, 1, 1, 1, 1, 2, True, "slots")
    rows = rc.length_sweep(size, buf)
    assert [r[0] for r in rows] == list(range(2, size + 1)) + [size] * rc.SWEEP_EXTRA_INSERTS
    buf.check_errors()


def _tagged_episodes(rng, n, T, N, D, S, A):
    """Random episodes whose first reward is the episode's number: a gathered batch names its indices."""
    ep = rc.episodes(rng, n, T, N, D, S, A)
    ep[3][0, :, 0, 0] = np.arange(n, dtype=np.float32)
    return ep


@pytest.mark.parametrize("size,n", [(16, 5), (2500, 2500)])
def test_uniform_device_rng(size, n):
    T, N, D, S, A, B, SEED = 3, 2, 5, 10, 3, 1000, 77
    rng = np.random.default_rng(size)
    buf = rc.make(False, size, T, N, D, S, A, True, seed=SEED)
    ora = RecBufferOracle(size, T, N, D, S, A, prioritized=False)
    ep = _tagged_episodes(rng, n, T, N, D, S, A)
    np.testing.assert_array_equal(buf.insert(n, *rc.as_dicts(ep)), ora.insert(n, *ep))
    seen = []
    for counter in (0, 1):
        want = rc.uniform_inds(SEED, counter, B, n)
        assert want.min() >= 0 and want.max() < n
        got = buf.sample(B)
        assert got[7] is None and got[8] is None
        tags = got[3][PID].cpu().numpy()[0, 0, :, 0]      # rewards [N, T, B, 1]
        np.testing.assert_array_equal(tags.astype(np.int64), want, err_msg=f"call {counter}")
        rc.compare_batch(got, ora.sample_inds(want), f"call {counter}")
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])
    assert len(np.unique(seen[0][768:])) > 1              # the partial last block draws too
    buf.check_errors()


@pytest.mark.parametrize("same_share", [True, False], ids=["same_share", "own_share"])
def test_insert_collected_second_pass(same_share):
    """The collector's fields through mm_erb_insert_concat, twice (the second insert wraps), against
    RecBufferOracle.insert of the same fields with share_obs = the agents' observations concatenated. The actions
    are all exploratory (epsilon 1), so the episodes differ from env to env after the first step whatever the
    policy."""
    from minimarl.env import VecEnv
    from minimarl.offq import OffQMix
    from minimarl.offq_runner import OffQCollector
    from minimarl.recbuf import RecReplayBuffer
    E, N, T, D, A, SIZE = 1400, 2, 3, 47, 5, 2000
    S = N * D
    assert (T + 1) * E * N * D > rc.GRID_SPAN
    tr = OffQMix(N, D, A, T, 8, mixer="vdn", seed=7)
    col = OffQCollector(VecEnv(E, N, max_steps=T, device="cuda"), tr, T, 1234)
    info = {PID: {"obs_space": (D,), "share_obs_space": (S,), "act_space": (A,)}}
    buf =RecReplayBuffer(info, {PID: list(range(N))}, SIZE, T, same_share, False, device="cuda")
    ora = RecBufferOracle(SIZE, T, N, D, S, A, prioritized=False, same_share=same_share)
    for it in range(2):
        fields, _, _ = col.collect(1.0)
        slots = buf.insert_collected(E, fields)
        h = {k: v.cpu().numpy() for k, v in fields.items()}
        cat = np.concatenate([h["obs"][:, :, a] for a in range(N)], -1)            # [T+1, E, N*D]
        share = np.repeat(cat[:, :, None, :], N, axis=2)                           # every agent sees the same row
        want = ora.insert(E, h["obs"], share, h["acts"], h["rewards"], h["dones"], h["dones_env"])
        np.testing.assert_array_equal(slots, want, err_msg=f"insert {it}")
        if it == 0:
            first_acts = h["acts"]
    np.testing.assert_array_equal(slots, (E + np.arange(E)) % SIZE)
    assert len(buf) == len(ora) == SIZE
    assert not np.array_equal(first_acts, h["acts"])      # the two collects differ (the counter moved on)
    # and so do the envs of one collect: 1400 uniform draws from 5 ** 6 action sequences collide about 63 times
    seqs = h["acts"].argmax(-1).transpose(1, 0, 2).reshape(E, -1)
    assert len(np.unique(seqs, axis=0)) > E // 2
    allidx = np.arange(SIZE)
    rc.compare_batch(buf.sample(SIZE, inds=allidx), ora.sample_inds(allidx), "whole ring")
    buf.check_errors()
