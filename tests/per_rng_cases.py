"""Cases and helpers shared by tests/test_per_rng_cpu.py (CPU) and tests/test_gpu_per_rng.py (GPU): the chunk
replay's samplers when they draw from the device counter RNG (csrc/per_small.h per_sample_body, csrc/per.hip
per_uniform_kernel), predicted draw for draw from oracle.rng and oracle.sumtree.

The stratified sampler's fraction for draw k of a call is (rng_draw(seed, counter + n_samples, k, 77) >> 11) * 2^-53,
the uniform sampler's the same with tag 91; n_samples is the device's count of sample calls so far. The GPU tests
copy the device tree into the oracle before every call (``mirror``), so both sides descend over bit-identical
nodes and nodes / slots are compared exactly; what is left to differ is s = a + (b - a) * f, which the kernel may
contract into an FMA (a move of about 2^-52 * root). ``descent_margin`` measures how close any comparison of any
draw comes to a node boundary, relative to the root: the exact comparison is valid while it stays above
MARGIN_MIN, which the CPU test asserts for every case on oracle-built trees and the GPU tests on the device's.
"""
import numpy as np

from oracle import rng as orng
from oracle.sumtree import SumTreeOracle

MARGIN_MIN = 1e-12        # >> 2^-52 (an FMA's move of s); the cases below keep >= 7.8e-10
WEIGHT_RTOL = 1e-5        # f32 IS weights against the f64 oracle (tests/test_gpu_rollout.py)
SEED, COUNTER, CALLS = 1234, 5, 3   # the counters reached: 5, 6, 7
# no seed had to be replaced: 1234 keeps the margin for every case below
SEEDS = (1234,)

# (flavor, cap, fill, B)
CASES = [
    ("qmix", 4, 3, 8),              # tree far smaller than the LDS top; more draws than leaves
    ("vdn", 1000, 700, 33),         # non-power-of-two capacity, partly filled, decay
    ("qmix", 1024, 1024, 1000),     # tree exactly the 2047-node top; last wave partial
    ("qmix", 2048, 2048, 1025),     # first level below the top; thread 0 owns a second sample
    ("vdn", 4099, 4099, 256),       # non-power-of-two capacity above the top
    ("qmix", 65536, 65536, 8192),   # the batch limit: eight samples per thread
]
CASE_IDS = [f"{f}-{c}-{n}-{b}" for f, c, n, b in CASES]

# the sample-ahead block of mm_clip_adam_pack: both flavors at one and at two samples per thread
PACK_CAP = 4096
PACK_CASES = [(f, PACK_CAP, PACK_CAP, b) for f in ("qmix", "vdn") for b in (32, 1025)]

# alpha_inc / beta_inc of about 1e-3: a doubled or missing anneal moves the weights by about 1e-3
ANNEAL = dict(max_episodes=50, update_iter=10)
_STEPS = ANNEAL["max_episodes"] * ANNEAL["update_iter"]
FLAVOR_KW = {
    "vdn": dict(alpha=0.4, beta=0.4, eps=1e-6, step_weight=0.99, use_step_weight=True),
    "qmix": dict(alpha=0.8, beta=0.2, eps=1e-6, step_weight=0.99, use_step_weight=False),
}


def make_oracle(flavor, cap):
    kw = FLAVOR_KW[flavor]
    return SumTreeOracle(cap, flavor, kw["alpha"], kw["beta"], kw["eps"], kw["step_weight"], kw["use_step_weight"],
                         alpha_inc=(1 - kw["alpha"]) / _STEPS, beta_inc=(1 - kw["beta"]) / _STEPS)


def make_device(flavor, cap):
    """A device PER with the oracle's settings (needs the GPU)."""
    from minimarl.replay import DevicePER
    return DevicePER(cap, flavor, device="cuda", update_alpha_beta=True, **FLAVOR_KW[flavor], **ANNEAL)


# The TDs' generator seed. Three leaves under eight strata leave the draws little to decide: with most TD sets
# the cap-4 case returns the same nodes on consecutive calls whatever the stream. Seed 2 is one where the three
# calls differ in every case (test_per_rng_cpu.py asserts it on the oracle), so "the batch differs from the previous
# call's" can be asked of the device everywhere.
TD_SEED = 2


def tds(fill):
    return (np.random.default_rng(TD_SEED).random(fill) * 3).astype(np.float32)


def filled_oracle(flavor, cap, fill):
    ora = make_oracle(flavor, cap)
    ora.add_batch([float(x) for x in tds(fill)])
    return ora


def filled_pair(flavor, cap, fill):
    import torch
    dev, ora = make_device(flavor, cap), make_oracle(flavor, cap)
    if fill:
        dev.add(torch.from_numpy(tds(fill)))
    return dev, ora


def n_samples(dev):
    return int(dev.device_scalars()[5])


def mirror(dev, ora):
    """The device's tree, fill count and annealed alpha / beta into the oracle."""
    ora.tree = dev.tree().cpu().numpy().copy()
    sc = dev.device_scalars()
    ora.n_data, ora.alpha, ora.beta = int(sc[0]), sc[1], sc[2]


def _descend(tree, B, fracs):
    """Every draw's descent a level at a time, in ``SumTreeOracle.sample``'s arithmetic:
    -> (smallest |s - tree[left]| over all comparisons, leaf nodes, the strata's s)."""
    n = len(tree)
    seg = tree[0] / B
    k = np.arange(B, dtype=np.float64)
    a, b = seg * k, seg * (k + 1)
    s0 = a + (b - a) * np.asarray(fracs, np.float64)
    s, idx, gap = s0.copy(), np.zeros(B, np.int64), np.inf
    while True:
        left = 2 * idx + 1
        live = left < n
        if not live.any():
            return gap, idx, s0
        lv = tree[np.where(live, left, 0)]
        gap = min(gap, float(np.abs(s - lv)[live].min()))
        go_left = s <= lv
        s = np.where(live & ~go_left, s - lv, s)
        idx = np.where(live, np.where(go_left, left, left + 1), idx)


def descent_margin(ora, B, fracs):
    """The smallest |s - tree[left]| / tree[0] over every comparison of every draw's descent."""
    return _descend(ora.tree, B, fracs)[0] / ora.tree[0]


def predict(ora, seed, ctr, B):
    """What a device-RNG sample call returns: (nodes, slots, priorities, IS weights); anneals the oracle and, for
    vdn, decays its tree, as the call does."""
    return ora.sample(B, orng.per_stratum_fracs(seed, ctr, B))
