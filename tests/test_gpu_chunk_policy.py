"""GPU: the chunk-persistent rollout's fp16x3 step loop runs the forward with a compile-time step policy (device draws
only, no q_out / training saves, Q head on tile 0, the role's epilogue behind a scalar branch), draws the eps-greedy
decisions of TWO steps per pass (even launch steps draw for themselves and for the next step; the odd step draws
nothing), and exchanges lanes in its epilogue with v_permlane16/32_swap and DPP instead of LDS shuffles. The fused
one-launch-per-step engine runs the generic policy with per-step draws, so everything the algorithm sees must stay
BIT-identical between the two engines built from the same seed.

Shapes: the rollout kernels need E >= 2048, so the smallest E whose last tile holds 44 envs (one partial 64-env group,
the others empty) is 9 x 256 + 44 = 2348; N = 3 is odd; chunk 4 with max_steps 5 puts chunk ends and auto-resets inside
the launches. Eager launches of 1, 2, 3, 5, 7 and 12 steps start at steps 0, 1, 3, 6, 11, 18: both parities, odd-length
launches (one spare draw), and a 1-step launch whose only step is also its last (its hidden-state write-back)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, N, CHUNK, MAX_STEPS = 2348, 3, 4, 5
SPANS = (1, 2, 3, 5, 7, 12)


def _pair(fgh, guard=False):
    from minimarl.engine import RolloutEngine
    f1, g, h = fgh
    kw = dict(f1=f1, g=g, h=h, chunk=CHUNK, capacity=2 * E, seed=41, max_steps=MAX_STEPS, device=DEV)
    a = RolloutEngine(E, N, fused=True, **kw)
    b = RolloutEngine(E, N, persistent=True, **kw)
    assert a.fused and not a.chunked and b.chunked and not b.fused
    assert (b.S - 1) * b.C >= max(SPANS)
    if guard:   # agent 1 beyond the fp16 range: both engines run it on the exact-f32 image
        for eng in (a, b):
            with torch.no_grad():
                eng.behavior.view("W1")[1, 0, :] = 3.0e3
            eng.behavior.mark_dirty()
            eng.sync_target()
    return a, b


def _step_arrays(e):
    """What the last executed step t - 1 left: its actions, Q(a), max Q', rewards, dones; the actions / Q(a) of step t
    (written one step ahead); both hidden states; the env state."""
    torch.cuda.synchronize()
    t = e.t
    if e.chunked:
        RL = e.RL
        st = [e.act_r[(t - 1) % RL], e.qsel_r[(t - 1) % RL], e.maxq_r[(t - 1) % RL], e.rew_r[(t - 1) % RL],
              e.done_r[(t - 1) % RL], e.act_r[t % RL], e.qsel_r[t % RL]]
    else:
        st = [e.act_buf[(t - 1) % 3], e.qsel_buf[(t - 1) % 3], e.maxq_buf[(t - 1) % 2], e.rew_buf[(t - 1) % 2],
              e.done_buf[(t - 1) % 2], e.act_buf[t % 3], e.qsel_buf[t % 3]]
    st += [e.h, e.ht, e.cur_row >= 0]
    return [x.detach().clone().cpu() for x in st] + [torch.as_tensor(v) for v in e.env.get_state()]


def _full_state(e):
    """The engine state as the algorithm sees it (tests/test_gpu_chunk.py `_state`): the chunk store through the PER's
    slot map and the staging map, hiddens, chunk_td, cur_row, the PER tree, the last step's outputs, the RNG counter."""
    torch.cuda.synchronize()
    rows = e.per.slot_rows().long()
    c = e.t % e.C
    stg = e.staging.long()
    st = [e.store.obs[rows], e.store.act[rows], e.store.rew[rows], e.store.done[rows],
          e.store.obs[stg, :c + 1] if c else e.store.obs[stg, :0], e.store.act[stg, :c], e.store.rew[stg, :c],
          e.store.done[stg, :c], e.h, e.ht, e.chunk_td, e.cur_row >= 0,
          e.per.tree(), e.act, e.last_rew, e.last_done, e.counter_dev[e.t % 2 if e.fused else 0]]
    return [x.detach().clone().cpu() for x in st] + [torch.as_tensor(v) for v in e.env.get_state()]


def _same(xs, ys, tag):
    assert len(xs) == len(ys)
    for i, (x, y) in enumerate(zip(xs, ys)):
        assert torch.equal(x, y), (tag, i)


def _run_spans(a, b, eps):
    b.set_epsilon(eps)
    for n in SPANS:
        t0 = b.t
        b._advance(n)                          # ONE eager launch of n steps
        assert b.t == t0 + n
        for _ in range(n):
            a.step(eps)
        _same(_step_arrays(a), _step_arrays(b), ("launch", t0, n))
    a.flush_td()
    assert a.t == b.t == sum(SPANS)
    _same(_full_state(a), _full_state(b), "end")
    b.check_errors()
    a.check_errors()


@pytest.mark.parametrize("eps", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("fgh", [(64, 64, 64), (64, 32, 32)])
def test_chunk_policy_eager_spans_bit_identical_to_fused(fgh, eps):
    a, b = _pair(fgh)
    _run_spans(a, b, eps)


def test_chunk_policy_guarded_agent_beside_specialised_blocks():
    """A range-guarded agent in every tile: its blocks run the exact-f32 loop (generic policy, per-step draws) beside
    the specialised fp16x3 blocks of the other agents."""
    a, b = _pair((64, 64, 64), guard=True)
    _run_spans(a, b, 0.3)


def test_chunk_policy_region_graph_bit_identical_to_fused():
    """Region graphs (capture_region / run_region): a 7-step launch entered at phase 3 (odd start, odd length, across
    two chunk ends) and a 6-step one from phase 10, against eager fused steps."""
    a, b = _pair((64, 64, 64))
    eps = 0.3
    for _ in range(3):
        b.step(eps)
    b.capture_region(7)
    b.run_region(7, eps)
    assert b.t == 10
    b.capture_region(6)
    b.run_region(6, eps)
    assert b.t == 16
    for _ in range(b.t):
        a.step(eps)
    _same(_step_arrays(a), _step_arrays(b), "regions")
    a.flush_td()
    _same(_full_state(a), _full_state(b), "end")
    b.check_errors()
    a.check_errors()
