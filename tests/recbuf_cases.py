"""Case scripts shared by tests/test_recbuf_sizes_cpu.py (CPU) and tests/test_gpu_recbuf_sizes.py (GPU): the
episode replay (csrc/recbuf.hip via minimarl.recbuf) at the sizes where its loops take a second pass.

Every script drives oracle.recbuf.RecBufferOracle and, when it is handed a device buffer, the device buffer
through the same calls, comparing as it goes; without one it runs the oracle alone and returns the facts the CPU
test asserts (so the GPU comparison is known not to compare infinities, empty leaves or constant weights).

Index comparisons are exact with nothing left out. A leaf is float32 prio ** alpha, where numpy's powf and the
device's pow may differ by one float32 ulp; at B = 1400 a sampled mass would now and then fall inside such a
sliver. ``sync_trees`` therefore, after every insert / update, checks the device's leaves against the oracle's
(rtol 4e-7, same finiteness), copies the device's leaves into the oracle's trees, re-derives every internal node
as op(v[2p], v[2p+1]) (what both sides define) and asserts the device's internal nodes BIT-equal. From there both
sides descend the same tree, so indices are compared with assert_array_equal; weights keep rtol 1e-6 (an f64
pow(-beta) through two libms); batches, ring slots, lengths and max_priority are bit-exact.

The device draws are predicted, not range-checked: oracle.rng restates rng_draw, the prioritized sampler uses
stream 0x5E6 and the uniform one 0x0E1 with (seed, call counter, b).
"""
import numpy as np

from oracle import rng as orng
from oracle.recbuf import RecBufferOracle, _reduce_ref

FIELDS = ("obs", "share_obs", "acts", "rewards", "dones", "dones_env")
PID = "policy_0"
TREE_RTOL = 4e-7          # one float32 ulp of prio ** alpha (tests/test_gpu_recbuf.py)
WEIGHT_RTOL = 1e-6
STREAM_PRIORITIZED, STREAM_UNIFORM = 0x5E6, 0x0E1

# big_ring: the smallest shape whose insert AND gather each move more than 2048 blocks x 256 threads = 524,288
# floats of one field, with more than 1024 leaves per insert and more than 1024 (and 256) draws per sample
BIG = dict(size=2500, T=3, N=2, D=47, S=94, A=5, alpha=0.6, seed=9, n_insert=1500, B=1400, inserts=3)
GRID_SPAN = 2048 * 256

# length_sweep: len - 2 on both sides of itcap / 2 - 1 for every itcap up to 64, and itcap == size
SWEEP_SIZES = (2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
SWEEP_FRACS = (1.0 - 2.0 ** -53, 0.0, 0.5)
SWEEP_EXTRA_INSERTS = 2   # past the full ring: the cursor wraps from ``size`` and overwrites slots 0, 1
# distinct float32 priorities, cycled by insert number: no two neighbouring leaves carry the same mass
PRIO_TABLE = np.array([0.3, 1.7, 0.9, 2.6, 0.45, 1.2, 3.3, 0.7, 2.1, 0.55, 1.45], np.float32)


class Box:
    def __init__(self, shape):
        self.shape = shape


class Discrete:
    def __init__(self, n):
        self.n = n


def make(prioritized, size, T, N, D, S, A, same_share=True, leaf_mode="reference", seed=0, alpha=0.6):
    """A device buffer (needs the GPU)."""
    from minimarl.recbuf import PrioritizedRecReplayBuffer, RecReplayBuffer
    pinfo = {PID: {"obs_space": Box((D,)), "share_obs_space": Box((S,)), "act_space": Discrete(A)}}
    pag = {PID: list(range(N))}
    if prioritized:
        return PrioritizedRecReplayBuffer(alpha, pinfo, pag, size, T, same_share, False, device="cuda", seed=seed,
                                          leaf_mode=leaf_mode)
    return RecReplayBuffer(pinfo, pag, size, T, same_share, False, device="cuda", seed=seed)


def episodes(rng, n, T, N, D, S, A):
    """n random episodes in the insert layout. share_obs is random per agent (not the observations repeated), so
    a same_share store must keep agent 0's row and a per-agent store every agent's own."""
    obs = rng.standard_normal((T + 1, n, N, D)).astype(np.float32)
    share = rng.standard_normal((T + 1, n, N, S)).astype(np.float32)
    acts = np.eye(A, dtype=np.float32)[rng.integers(0, A, (T, n, N))]
    rew = rng.standard_normal((T, n, N, 1)).astype(np.float32)
    dones = (rng.random((T, n, N, 1)) < 0.1).astype(np.float32)
    de = (rng.random((T, n, 1)) < 0.1).astype(np.float32)
    return obs, share, acts, rew, dones, de


def as_dicts(ep):
    return [{PID: x} for x in ep]


def u53(seed, counter, B, stream):
    """(rng_draw(seed, counter, b, stream) >> 11) / 2**53 for b < B (recbuf.hip rng_unit53), exact in float64."""
    r = orng.rng_draw(np.uint64(seed), np.uint64(counter), np.arange(B, dtype=np.uint64), np.uint64(stream))
    return (r >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def device_fracs(seed, counter, B):
    """What the prioritized sampler draws when no ``fracs`` are injected."""
    return u53(seed, counter, B, STREAM_PRIORITIZED)


def uniform_inds(seed, counter, B, length):
    """What the uniform sampler draws: min(floor(u53 * len), len - 1)."""
    k = np.floor(u53(seed, counter, B, STREAM_UNIFORM) * np.float64(length)).astype(np.int64)
    return np.minimum(k, length - 1)


def tree_close(a, b, what):
    fin = np.isfinite(b)
    np.testing.assert_array_equal(np.isfinite(a), fin, err_msg=what)
    np.testing.assert_allclose(a[fin], b[fin], rtol=TREE_RTOL, atol=0, err_msg=what)


def rederive(tree):
    """Every internal node from the leaves: v[p] = op(v[2p], v[2p+1]) for p = cap - 1 .. 1, a level at a time."""
    w = tree.cap // 2
    while w >= 1:
        p = np.arange(w, 2 * w)
        tree.v[p] = tree.op(tree.v[2 * p], tree.v[2 * p + 1])
        w //= 2


def sync_trees(buf, ora, what):
    """See the module docstring. One device read (``state()``) per call; returns the error word."""
    s, m, maxp, err = [t.cpu().numpy() for t in buf.state()]
    cap = ora.sum.cap
    assert s.shape == m.shape == (2 * cap,), what
    for dev, tree in ((s, ora.sum), (m, ora.min)):
        name = f"{what}: {tree.kind} tree"
        tree_close(dev[cap:], tree.v[cap:], name + " leaves")
        tree.v[cap:] = dev[cap:]
        rederive(tree)
        np.testing.assert_array_equal(dev[:cap], tree.v[:cap], err_msg=name + " internal nodes")
    assert np.float32(maxp[0]) == np.float32(ora.max_p), (what, maxp[0], ora.max_p)
    return int(err[0])


def compare_sample(got, batch, w, idx, what):
    """A device prioritized sample (the 9-tuple) against the oracle's (batch, weights, idx)."""
    np.testing.assert_array_equal(got[8].cpu().numpy(), idx, err_msg=what + " idx")
    np.testing.assert_allclose(got[7].cpu().numpy(), w, rtol=WEIGHT_RTOL, atol=0, err_msg=what + " weights")
    compare_batch(got, batch, what)


def compare_batch(got, batch, what):
    for k, x, y in zip(FIELDS, got[:6], batch):
        np.testing.assert_array_equal(x[PID].cpu().numpy(), y, err_msg=f"{what} {k}")


def gather_ring(buf, inds):
    """sample_inds on any device buffer (the prioritized class has no ``inds=``; the base class's sample does)."""
    from minimarl.recbuf import RecReplayBuffer
    return RecReplayBuffer.sample(buf, len(inds), inds=np.asarray(inds, np.int64))


def crosses(idx, at):
    """Does some value of idx occur both before position ``at`` and at or after it?"""
    return np.intersect1d(idx[:at], idx[at:]).size > 0


def big_ring(leaf_mode, same_share, buf=None):
    """Three wrapping 1500-episode inserts into a 2500 ring; after each: a 1400-draw sample by the device RNG, an
    update with the sampled (duplicate-laden) indices, and a second sample that sees the new priorities.
    Returns the oracle-side facts per insert."""
    import torch
    c = BIG
    dims = (c["T"], c["N"], c["D"], c["S"], c["A"])
    ora = RecBufferOracle(c["size"], *dims, alpha=c["alpha"], prioritized=True, leaf_mode=leaf_mode,
                          same_share=same_share)
    rng = np.random.default_rng(21)
    n, B = c["n_insert"], c["B"]
    counter = 0
    facts = dict(fracs=[], first_w=[], second_w=[], idx=[], current=[], moved=[])
    for it in range(c["inserts"]):
        what = f"insert {it}"
        ep = episodes(rng, n, *dims)
        facts["current"].append(ora.current)
        slots = ora.insert(n, *ep)
        facts["moved"].append(ep[0].size)
        if buf is not None:
            np.testing.assert_array_equal(buf.insert(n, *as_dicts(ep)), slots, err_msg=what)
            assert len(buf) == len(ora)
            sync_trees(buf, ora, what)
        for phase in ("first", "second"):
            beta = 0.4 + 0.1 * it + (0.05 if phase == "second" else 0.0)
            fr = device_fracs(c["seed"], counter, B)       # counter: RecReplayBuffer._next_counter
            counter += 1
            got = buf.sample(B, beta, PID) if buf is not None else None
            batch, w, idx = ora.sample(B, beta, fr)
            facts["fracs"].append(fr)
            facts[phase + "_w"].append(w)
            if buf is not None:
                compare_sample(got, batch, w, idx, f"{what} {phase} sample")
            if phase == "second":
                break
            facts["idx"].append(idx)
            prio = (0.05 + 3.0 * rng.random(B)).astype(np.float32)
            ora.update_priorities(idx, prio)
            if buf is not None:
                buf.update_priorities(got[8], torch.as_tensor(prio).cuda(), PID)
                sync_trees(buf, ora, what + " update")
    if buf is not None:
        buf.check_errors()
    return facts


def sweep_priority(i):
    return PRIO_TABLE[i % len(PRIO_TABLE)]


def length_sweep(size, buf=None):
    """Slots mode, one episode per insert, the inserted slot's priority set from PRIO_TABLE; at every length >= 2
    a sample of min(3, len - 1) with SWEEP_FRACS. Returns per sample (len, idx, weights, fold, fold by recursion)."""
    import torch
    T = N = D = S = 1
    A = 2
    ora = RecBufferOracle(size, T, N, D, S, A, alpha=0.6, prioritized=True, leaf_mode="slots")
    rng = np.random.default_rng(100 + size)
    out = []
    for i in range(size + SWEEP_EXTRA_INSERTS):
        what = f"size {size} insert {i}"
        ep = episodes(rng, 1, T, N, D, S, A)
        slot = ora.insert(1, *ep)
        prio = np.array([sweep_priority(i)], np.float32)
        ora.update_priorities(slot, prio)
        if buf is not None:
            np.testing.assert_array_equal(buf.insert(1, *as_dicts(ep)), slot, err_msg=what)
            buf.update_priorities(torch.as_tensor(slot).cuda(), torch.as_tensor(prio).cuda(), PID)
            assert len(buf) == len(ora)
            assert sync_trees(buf, ora, what) == 0
        ln = len(ora)
        if ln < 2:
            continue
        B = min(3, ln - 1)
        fr = np.array(SWEEP_FRACS[:B], np.float64)
        batch, w, idx = ora.sample(B, 0.5, fr)
        if buf is not None:
            compare_sample(buf.sample(B, 0.5, PID, fracs=fr), batch, w, idx, what)
        out.append((ln, idx, w, ora.sum.reduce_prefix(ln - 2), _reduce_ref(ora.sum, ln - 2)))
    return out
