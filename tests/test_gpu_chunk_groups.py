"""GPU: the chunk-persistent rollout's fp16x3 step loop runs a block's 256 envs as four independent 64-env groups
(waves 4j .. 4j + 3, envs 64j .. 64j + 63 of the tile) with no block barrier per step, so inside a multi-step launch
the groups of a block, and of the tile's other blocks, drift apart. tests/test_gpu_chunk.py runs its multi-step
launches at E = 2048 only (every group full) and its partial tiles with one-step launches only; here multi-step
launches run on tiles whose last groups are partial or empty, on a tile that mixes fp16x3 and exact-f32 blocks (the
exact body keeps its block-synchronous loop and publishes all 32 hand-off words at once) and across chunk starts and
auto-resets inside a launch. As there, everything the algorithm sees must be BIT-identical to the fused
one-launch-per-step engine with the same seed."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _state(e):
    """The engine state as the algorithm sees it (tests/test_gpu_chunk.py `_state`): store rows through the PER's
    slot map and the staging map, hiddens, priorities, rings, RNG counter, env state."""
    torch.cuda.synchronize()
    rows = e.per.slot_rows().long()
    c = e.t % e.C
    stg = e.staging.long()
    st = [e.store.obs[rows], e.store.act[rows], e.store.rew[rows], e.store.done[rows],
          e.store.obs[stg, :c + 1] if c else e.store.obs[stg, :0], e.store.act[stg, :c], e.store.rew[stg, :c],
          e.store.done[stg, :c], e.h, e.ht, e.chunk_td, e.cur_row >= 0,
          e.per.tree(), e.act, e.last_rew, e.last_done, e.counter_dev[e.t % 2 if e.fused else 0]]
    return [x.detach().clone().cpu() for x in st] + [torch.as_tensor(v) for v in e.env.get_state()]


def _pair(E, n, f1, g, h, guard, chunk, max_steps):
    from minimarl.engine import RolloutEngine
    kw = dict(f1=f1, g=g, h=h, chunk=chunk, capacity=2 * E, seed=37, max_steps=max_steps, device=DEV)
    a = RolloutEngine(E, n, fused=True, **kw)
    b = RolloutEngine(E, n, persistent=True, **kw)
    assert a.fused and not a.chunked and b.chunked and not b.fused
    if guard:   # agent 3 beyond the fp16 range: both engines run it on the exact-f32 image
        for eng in (a, b):
            with torch.no_grad():
                eng.behavior.view("W1")[3, 0, :] = 3.0e3
            eng.behavior.mark_dirty()
            eng.sync_target()
    return a, b


def _same(a, b, tag):
    for i, (x, y) in enumerate(zip(_state(a), _state(b))):
        assert torch.equal(x, y), (tag, i)


# E, N, (f1, g, h), guard, chunk, max_steps: the last tile holds
#   2100: 52 envs (one partial group, three empty)          2200: 152 envs (two full groups, 24 envs, one empty)
#   2048: full, blocks of both bodies in every tile         2304: full; chunk starts and resets inside the launches
CASES = [(2100, 4, (64, 64, 64), False, 10, 100),
         (2200, 8, (64, 32, 32), False, 10, 100),
         (2048, 8, (64, 64, 64), True, 10, 100),
         (2304, 4, (64, 64, 64), False, 17, 5)]


@pytest.mark.parametrize("E,n,fgh,guard,chunk,max_steps", CASES)
def test_chunk_groups_multi_step_launches_bit_identical_to_fused(E, n, fgh, guard, chunk, max_steps):
    """Single steps to phase 3, ONE 20-step launch (a region graph entered at phase 3), single steps, ONE 30-step
    launch (the longest span of a chunk-10 engine: (S - 1) C), single steps — against eager fused steps."""
    a, b = _pair(E, n, *fgh, guard, chunk, max_steps)
    assert (b.S - 1) * b.C >= 30
    eps = 0.3
    for _ in range(3):
        b.step(eps)                            # phase 0..2: one-step launches
    b.capture_region(20)
    b.run_steps(20, eps)                       # phase 3: one launch of 20 steps
    assert b.t == 23
    for _ in range(4):
        b.step(eps)                            # phase 23..26
    b.capture_region(30)
    b.run_steps(30, eps)                       # phase 27: one launch of 30 steps
    assert b.t == 57
    for _ in range(3):
        b.step(eps)
    for _ in range(b.t):
        a.step(eps)
    a.flush_td()
    assert a.t == b.t == 60
    _same(a, b, "end")
    b.check_errors()
    a.check_errors()
