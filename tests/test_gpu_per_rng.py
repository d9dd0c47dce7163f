"""The chunk replay's samplers on their production paths, where the draws come from the device counter RNG,
against oracle.rng + oracle.sumtree (helpers and cases: tests/per_rng_cases.py):

* mm_per_sample_rng (eager and graph updates), mm_per_sample_uniform (qmix_min replay) and the sample-ahead
  block of mm_clip_adam_pack (multi-update graphs), called directly;
* the same through QLearner.update, capture_update / replay_update and update_uniform.

Every call's stream is (seed, counter argument + n_samples): the device's call counter is what gives a replayed
graph a fresh batch, so each test reads it, predicts the batch from it and checks it advanced by one. Nodes and
slots are exact (the oracle descends a copy of the device tree; the margin that makes this valid is asserted and
printed per call), IS weights rtol 1e-5.
"""
import ctypes

import numpy as np
import pytest
import torch

import per_rng_cases as pc
from oracle import rng as orng

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED, COUNTER = pc.SEED, pc.COUNTER


def _np(t):
    return t.cpu().numpy()


def _margin(ora, seed, ctr, B, what):
    m = pc.descent_margin(ora, B, orng.per_stratum_fracs(seed, ctr, B))
    print(f"{what}: ctr {ctr} B {B} margin {m:.3e}")
    assert m >= pc.MARGIN_MIN, what
    return m


def _restored(flavor, cap, ts):
    per = pc.make_device(flavor, cap)
    per.restore_tensors(ts)
    return per


@pytest.mark.parametrize("flavor,cap,fill,B", pc.CASES, ids=pc.CASE_IDS)
def test_sample_rng_vs_oracle(flavor, cap, fill, B):
    dev, ora = pc.filled_pair(flavor, cap, fill)
    prev = None
    for call in range(pc.CALLS):
        pc.mirror(dev, ora)
        ns = pc.n_samples(dev)
        assert ns == call and ora.n_data == fill
        before = ora.tree.copy()
        _margin(ora, SEED, COUNTER + ns, B, f"{flavor} cap {cap} call {call}")
        on, oslots, _, ow = pc.predict(ora, SEED, COUNTER + ns, B)
        nodes, slots, w = dev.sample(B, seed=SEED, counter=COUNTER)
        nodes, slots, w = _np(nodes), _np(slots), _np(w)
        np.testing.assert_array_equal(nodes, on)
        np.testing.assert_array_equal(slots, oslots)
        np.testing.assert_allclose(w, ow, rtol=pc.WEIGHT_RTOL)
        sc = dev.device_scalars()
        assert sc[1] == ora.alpha and sc[2] == ora.beta          # annealed once, before the draws
        assert int(sc[5]) == ns + 1 and int(sc[0]) == fill
        assert slots.min() >= 0 and slots.max() < fill
        if prev is not None:
            assert not np.array_equal(nodes, prev)
        prev = nodes
        after = _np(dev.tree())
        if flavor == "vdn":                                      # decayed after the draws
            np.testing.assert_allclose(after, ora.step_weight * before, rtol=1e-15, atol=0)
        else:
            np.testing.assert_array_equal(after, before)


def test_sample_rng_refusals():
    dev, _ = pc.filled_pair("qmix", 16384, 16384)
    with pytest.raises(RuntimeError, match="batch must be in"):
        dev.sample(8193, seed=SEED, counter=COUNTER)
    assert pc.n_samples(dev) == 0                                # nothing ran
    dev.sample(8192, seed=SEED, counter=COUNTER)                 # the limit itself is accepted
    assert pc.n_samples(dev) == 1
    empty, _ = pc.filled_pair("qmix", 64, 0)
    with pytest.raises(RuntimeError, match="empty buffer"):
        empty.sample(8, seed=SEED, counter=COUNTER)
    assert pc.n_samples(empty) == 0 and empty.device_scalars()[2] == pc.FLAVOR_KW["qmix"]["beta"]


def test_counter_argument_adds_to_call_count():
    """Counter 6 at n_samples 0 is the stream of counter 5 at n_samples 1 (qmix: the first call leaves the tree
    alone; it anneals beta, so only nodes and slots are the same)."""
    cap, fill, B = 2048, 2048, 1025
    src, _ = pc.filled_pair("qmix", cap, fill)
    ts, _ = src.checkpoint_tensors()
    a, b = _restored("qmix", cap, ts), _restored("qmix", cap, ts)
    na, sa, _ = a.sample(B, seed=SEED, counter=COUNTER + 1)
    first, _, _ = b.sample(B, seed=SEED, counter=COUNTER)
    assert pc.n_samples(b) == 1
    nb, sb, _ = b.sample(B, seed=SEED, counter=COUNTER)
    np.testing.assert_array_equal(_np(na), _np(nb))
    np.testing.assert_array_equal(_np(sa), _np(sb))
    assert not np.array_equal(_np(first), _np(nb))


@pytest.mark.parametrize("flavor,cap,fill,B", [pc.CASES[1], pc.CASES[3]], ids=[pc.CASE_IDS[1], pc.CASE_IDS[3]])
def test_checkpoint_carries_call_count(flavor, cap, fill, B):
    dev, ora = pc.filled_pair(flavor, cap, fill)
    for _ in range(2):
        dev.sample(B, seed=SEED, counter=COUNTER)
    ts, _ = dev.checkpoint_tensors()
    assert int(ts["scalars"][5]) == 2
    fresh = _restored(flavor, cap, ts)
    assert pc.n_samples(fresh) == 2
    pc.mirror(fresh, ora)
    _margin(ora, SEED, COUNTER + 2, B, f"checkpoint {flavor}")
    on, oslots, _, ow = pc.predict(ora, SEED, COUNTER + 2, B)
    outs = [[_np(x) for x in p.sample(B, seed=SEED, counter=COUNTER)] for p in (dev, fresh)]
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(outs[0][0], on)
    np.testing.assert_array_equal(outs[0][1], oslots)
    np.testing.assert_allclose(outs[0][2], ow, rtol=pc.WEIGHT_RTOL)
    assert fresh.device_scalars() == dev.device_scalars()
    assert torch.equal(fresh.tree(), dev.tree())


@pytest.mark.parametrize("B", [1000, 32])
@pytest.mark.parametrize("fill", [5, 2500])
def test_sample_uniform_vs_oracle(fill, B):
    from minimarl._lib import check, lib
    from minimarl.qnet import ptr, stream_handle
    cap, seed, counter = 4096, 77, 3
    dev, _ = pc.filled_pair("qmix", cap, fill)
    tree0, sc0 = dev.tree(), dev.device_scalars()
    s = stream_handle(torch.device(DEV))
    seen = []
    for call in range(2):
        ns = pc.n_samples(dev)
        assert ns == call
        slots = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        w = torch.zeros(B, device=DEV)
        check(lib().mm_per_sample_uniform(dev._h, B, seed, counter, ptr(slots), ptr(w), s), "per_sample_uniform")
        want = orng.per_uniform_slots(seed, counter + ns, B, fill)
        assert want.min() >= 0 and want.max() < fill
        np.testing.assert_array_equal(_np(slots), want)
        np.testing.assert_array_equal(_np(w), np.ones(B, np.float32))
        sc = dev.device_scalars()
        assert sc[:5] == sc0[:5] and int(sc[5]) == ns + 1        # fill, alpha, beta untouched; one more call
        assert torch.equal(dev.tree(), tree0)
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])
    if B == 1000:
        assert len(np.unique(_np(slots)[768:])) > 1              # the draws of the partial last pass


def _adam_problem():
    """The net, parameters and random gradients of test_gpu_learner.py::test_clip_adam_pack_matches_separate_calls."""
    from minimarl.qnet import AgentQNet
    N, D, A = 8, 47, 5
    net = AgentQNet(N, D, A, 64, 64, 64, DEV, seed=5)
    n_agent, n_mix = net.n_params, 9000
    n = n_agent + n_mix
    g = torch.Generator().manual_seed(11)
    P0 = torch.randn(n, generator=g) * 0.1
    G0 = torch.randn(n, generator=g) * 0.05
    m0 = torch.randn(n, generator=g) * 1e-3
    v0 = torch.rand(n, generator=g) * 1e-4
    return net, n, n_agent, (P0, G0, m0, v0)


class _AdamSide:
    def __init__(self, net, n, n_agent, init):
        from minimarl.qnet import ptr
        self.P, self.G, self.m, self.v = (x.clone().to(DEV) for x in init)
        self.step = torch.full((1,), 2.0, device=DEV)
        self.partials = torch.zeros(512, device=DEV)
        self.norm = torch.zeros(2, device=DEV)
        self.packed = torch.zeros_like(net.packed)
        self.img = (net.packed.numel() - ((net.N + 63) & ~63)) // 2     # the f32 image
        self.head = (ptr(self.P), ptr(self.G), ptr(self.m), ptr(self.v), n, n_agent, 0,
                     5.0, 1e-3, 0.9, 0.999, 1e-8, ptr(self.step), ptr(self.partials), ptr(self.norm), 1.0,
                     ctypes.byref(net.dims), ptr(self.packed))

    def state(self):
        return [self.P, self.m, self.v, self.step, self.norm, self.packed[:self.img]]


@pytest.mark.parametrize("flavor,cap,fill,B", pc.PACK_CASES, ids=[f"{c[0]}-{c[3]}" for c in pc.PACK_CASES])
def test_clip_adam_pack_sample_ahead_vs_oracle(flavor, cap, fill, B):
    """One mm_clip_adam_pack launch whose extra block draws the next batch (next_per) against the same step with no
    PER followed by mm_per_sample_rng: bit-equal on every output, and the batch is the oracle's."""
    from minimarl._lib import check, lib
    from minimarl.qnet import ptr, stream_handle
    L, s = lib(), stream_handle(torch.device(DEV))
    net, n, n_agent, init = _adam_problem()
    src, ora = pc.filled_pair(flavor, cap, fill)
    src.sample(B, seed=SEED, counter=COUNTER)                    # n_samples = 1 in the checkpoint
    ts, _ = src.checkpoint_tensors()
    pers = [_restored(flavor, cap, ts) for _ in range(2)]
    pc.mirror(pers[0], ora)
    assert pc.n_samples(pers[0]) == 1
    _margin(ora, SEED, COUNTER + 1, B, f"adam_pack {flavor}")
    on, oslots, _, ow = pc.predict(ora, SEED, COUNTER + 1, B)
    res = []
    for fused, per in zip((True, False), pers):
        side = _AdamSide(net, n, n_agent, init)
        nodes = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        slots = torch.full((B,), -1, dtype=torch.int64, device=DEV)
        isw = torch.zeros(B, device=DEV)
        if fused:
            check(L.mm_clip_adam_pack(*side.head, None, None, None, B, per._h, SEED, COUNTER, ptr(nodes), ptr(slots),
                                      ptr(isw), s), "clip_adam_pack")
        else:
            check(L.mm_clip_adam_pack(*side.head, None, None, None, 0, None, 0, 0, None, None, None, s),
                  "clip_adam_pack")
            check(L.mm_per_sample_rng(per._h, B, SEED, COUNTER, ptr(nodes), ptr(slots), ptr(isw), s),
                  "per_sample_rng")
        torch.cuda.synchronize()
        res.append(side.state() + [nodes, slots, isw, per.tree(),
                                   torch.tensor(per.device_scalars(), dtype=torch.float64)])
    for x, y in zip(*res):
        assert torch.equal(x, y)
    assert res[0][3].item() == 3.0 and res[0][4][0] > 5.0        # one Adam step, the clip engaged
    np.testing.assert_array_equal(_np(res[0][6]), on)
    np.testing.assert_array_equal(_np(res[0][7]), oslots)
    np.testing.assert_allclose(_np(res[0][8]), ow, rtol=pc.WEIGHT_RTOL)
    sc = pers[0].device_scalars()
    assert int(sc[5]) == 2 and sc[1] == ora.alpha and sc[2] == ora.beta


def test_clip_adam_pack_sample_ahead_refusals():
    """A priority update and a sample-ahead in one launch, and a sample-ahead from an empty PER, are refused before
    anything is launched: parameters, the Adam step and the PER stay as they were."""
    from minimarl._lib import lib
    from minimarl.qnet import ptr, stream_handle
    L, s = lib(), stream_handle(torch.device(DEV))
    net, n, n_agent, init = _adam_problem()
    B, cap = 32, pc.PACK_CAP
    per, _ = pc.filled_pair("qmix", cap, cap)
    empty, _ = pc.filled_pair("qmix", cap, 0)
    side = _AdamSide(net, n, n_agent, init)
    nodes = torch.randint(cap - 1, 2 * cap - 1, (B,), generator=torch.Generator().manual_seed(1)).to(DEV)
    td = torch.rand(B, generator=torch.Generator().manual_seed(2)).to(DEV)
    out_n = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    out_s = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    isw = torch.zeros(B, device=DEV)
    tree0 = per.tree()
    tail = (SEED, COUNTER, ptr(out_n), ptr(out_s), ptr(isw), s)
    assert L.mm_clip_adam_pack(*side.head, per._h, ptr(nodes), ptr(td), B, per._h, *tail) != 0
    assert b"no priority update" in L.mm_last_error()
    assert L.mm_clip_adam_pack(*side.head, None, None, None, B, empty._h, *tail) != 0
    assert b"empty buffer" in L.mm_last_error()
    assert L.mm_clip_adam_pack(*side.head, None, None, None, 8193, per._h, *tail) != 0
    torch.cuda.synchronize()
    assert side.step.item() == 2.0 and torch.equal(side.P.cpu(), init[0])
    assert (out_n == -1).all() and (out_s == -1).all()
    assert torch.equal(per.tree(), tree0) and pc.n_samples(per) == 0 and pc.n_samples(empty) == 0
    assert per.device_scalars()[2] == pc.FLAVOR_KW["qmix"]["beta"]


def _engine_learner(mode="qmix", f1=64, g=64, h=64):
    """The engine and learner of test_gpu_learner.py::test_learner_update_from_device_per (E 128, N 4, B 32)."""
    from minimarl.engine import RolloutEngine
    from minimarl.learner import Mixer, QLearner
    E, N = 128, 4
    eng = RolloutEngine(E, N, f1=f1, g=g, h=h, chunk=10, capacity=512, seed=5, device=DEV,
                        per_kwargs=dict(update_alpha_beta=True, **pc.FLAVOR_KW["qmix"], **pc.ANNEAL))
    for _ in range(3):
        eng.run_graph(0.5)
    mix = Mixer(N, N * eng.D, 64, 32, DEV, seed=1)
    tmix = Mixer(N, N * eng.D, 64, 32, DEV, seed=1)
    L = QLearner(eng.behavior, eng.target, mix, tmix, batch=32, chunk=10, mode=mode, device=DEV)
    torch.cuda.synchronize()
    return eng, L


def _engine_oracle(eng):
    """An oracle of the engine PER's flavor and capacity (``mirror`` supplies the tree, alpha and beta)."""
    ora = pc.make_oracle("qmix", eng.per.capacity)
    sc = eng.per.device_scalars()
    assert (sc[3], sc[4]) == (ora.alpha_inc, ora.beta_inc)
    return ora


def _learner_batch_matches(L, eng, ora, seed, ctr, what):
    pc.mirror(eng.per, ora)
    _margin(ora, seed, ctr, L.B, what)
    return pc.predict(ora, seed, ctr, L.B)


def test_learner_eager_updates_draw_the_predicted_batches():
    eng, L = _engine_learner()
    ora = _engine_oracle(eng)
    prev = None
    for k in range(3):
        ns = pc.n_samples(eng.per)
        assert ns == k
        on, oslots, _, ow = _learner_batch_matches(L, eng, ora, 9, k + ns, f"eager update {k}")
        L.update(eng.per, eng.store, eng.env.reset_obs_ptr(), seed=9, counter=k)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(L.nodes), on)
        np.testing.assert_array_equal(_np(L.slots), oslots)
        np.testing.assert_allclose(_np(L.isw).ravel(), ow, rtol=pc.WEIGHT_RTOL)
        assert pc.n_samples(eng.per) == ns + 1
        assert oslots.max() < len(eng.per)
        if prev is not None:
            assert not np.array_equal(on, prev)
        prev = on
    assert np.isfinite(L.loss.item())


def test_learner_graph_replays_draw_afresh():
    """A replayed graph holds the same kernel arguments every time: only the device's call counter moves its
    stream on. Capturing records kernels without running them, so it leaves the counter alone."""
    eng, L = _engine_learner()
    ora = _engine_oracle(eng)
    n0 = pc.n_samples(eng.per)
    tree0 = eng.per.tree()
    L.capture_update(eng.per, eng.store, eng.env.reset_obs_ptr(), seed=5)
    torch.cuda.synchronize()
    assert pc.n_samples(eng.per) == n0 == 0
    assert torch.equal(eng.per.tree(), tree0)
    prev = None
    for k in range(3):
        ns = pc.n_samples(eng.per)
        assert ns == n0 + k
        on, oslots, _, ow = _learner_batch_matches(L, eng, ora, 5, ns, f"replay {k}")
        L.replay_update()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(L.nodes), on)
        np.testing.assert_array_equal(_np(L.slots), oslots)
        np.testing.assert_allclose(_np(L.isw).ravel(), ow, rtol=pc.WEIGHT_RTOL)
        assert pc.n_samples(eng.per) == ns + 1
        if prev is not None:
            assert not np.array_equal(on, prev)
        prev = on
    assert np.isfinite(L.loss.item())


def test_learner_uniform_updates_draw_the_predicted_slots():
    eng, L = _engine_learner("qmix_min", f1=128, g=32, h=32)
    fill = len(eng.per)
    assert int(eng.per.device_scalars()[0]) == fill
    seen = []
    for k in range(2):
        ns = pc.n_samples(eng.per)
        assert ns == k
        L.update_uniform(eng.per, eng.store, eng.env.reset_obs_ptr(), seed=3, counter=7)
        torch.cuda.synchronize()
        want = orng.per_uniform_slots(3, 7 + ns, L.B, fill)
        np.testing.assert_array_equal(_np(L.slots), want)
        assert pc.n_samples(eng.per) == ns + 1
        seen.append(want)
    assert not np.array_equal(seen[0], seen[1])
