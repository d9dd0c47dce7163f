"""CPU: MAPPO at the Switch2 observation width (obs_dim 3; critic width 3, or 6 with use_centralized_V over the 2
agents). Pins the restatements the GPU tests compare with -- oracle.mappo with tests/mappo_mb_ref.py /
mappo_cv_ref.py (recurrent) and tests/mappo_ff_ref.py (feed-forward), generic in the input width and used unchanged
-- to the reference's goldens at that width (tests/golden/mappo_sw_*.npz, make_golden_mappo_switch.py), and checks
the host side of the C ABI for the new shapes: parameter layout, scratch counts, the refusal of unbuilt (3, n)."""
import ctypes

import numpy as np
import pytest
import torch

import mappo_mb_ref as mb
import mappo_sw_cases as sw
from oracle import mappo as om

TOL = dict(rtol=1e-5, atol=2e-6)   # forward values, log-probs and hiddens (tests/test_gpu_mappo.py)


@pytest.mark.parametrize("name", list(sw.FWD_CASES))
def test_forward_reproduces_the_golden(name):
    """get_actions with the recorded actions and get_values on the same inputs; the agents of an env share the
    clock, and with the 6-wide critic their whole input, yet the recurrent critic's values differ (own hiddens)."""
    recurrent, cent = sw.FWD_CASES[name]
    fx = sw.fwd_case(name)
    assert fx["obs"].shape == (12, 3) and fx["critic.base.feature_norm.weight"].shape == (6 if cent else 3,)
    assert sorted(k for k in fx if k.startswith("actor.")) == sorted("actor." + om.ref_name(k, "actor")
                                                                      for k in sw.keys(recurrent))
    v, lp, ha, hc = sw.fwd_oracle(fx, recurrent, cent)
    np.testing.assert_allclose(v.numpy(), fx["values"], **TOL)
    np.testing.assert_allclose(v.numpy(), fx["get_values"], **TOL)
    np.testing.assert_allclose(lp.numpy(), fx["logp"], **TOL)
    np.testing.assert_allclose(ha.numpy(), fx["ha_out"][:, 0], **TOL)
    np.testing.assert_allclose(hc.numpy(), fx["hc_out"][:, 0], **TOL)
    obs = fx["obs"].reshape(6, 2, 3)
    assert np.array_equal(obs[:, 0, 2], obs[:, 1, 2]) and set(np.unique(obs[..., 0])) <= {0.0, 0.5, 1.0}


@pytest.mark.parametrize("run", ["m1", "m2"])
@pytest.mark.parametrize("name", list(sw.TRAIN_CASES))
def test_oracle_loop_reproduces_the_golden_train(name, run):
    """The fp32 loop on the recorded permutations (E 4, N 2, T 10, L 5, 3 epochs: 16 chunks / 80 rows; m2: two
    minibatches of 8 chunks / 40 rows): post-train parameters, ValueNorm state and (m1) the first update's gradients
    within K_FP32 fp32 spreads plus the golden's own distance to the f64 run; pre-clip norms and mean ratio at
    rtol 1e-5."""
    _, _, recurrent, cent = sw.TRAIN_CASES[name]
    fx, (o64, spread), (g64, gspread), o32, g32 = sw.oracle_case(name, run)
    M, EP = int(fx["train_batch_size"]), int(fx["epochs"])
    units = 16 if recurrent else 80
    assert (M, fx["perms"].shape, fx["norms"].shape) == (1 if run == "m1" else 2, (EP, units), (2 * EP * M,))
    assert fx["before.critic.base.mlp.fc1.0.weight"].shape == (32, 6 if cent else 3)
    assert (fx["data.active_masks"] == 0).sum() == 1 and (fx["data.masks"] == 0).sum() == 6
    for kind in ("actor", "critic"):
        for k in sw.keys(recurrent):
            after = fx[f"after.{kind}.{om.ref_name(k, kind)}"]
            mb.assert_within(o32[(kind, k)], after, spread[(kind, k)], f"{kind} {k} vs golden",
                             float(np.abs(after - o64[(kind, k)]).max()))
    if run == "m1":
        for n in (0, 1):
            for k in sw.keys(recurrent):
                ref = mb.golden_grad(fx, 0, n, k)
                mb.assert_within(g32[(0, n, k)], ref, gspread[(0, n, k)], f"update 0 net {n} {k} vs golden",
                                 float(np.abs(ref - g64[(0, n, k)]).max()))
    np.testing.assert_allclose(o32["norms"], fx["norms"], rtol=1e-5)
    for key, gk in (("vn_mean", "vn1.running_mean"), ("vn_mean_sq", "vn1.running_mean_sq")):
        mb.assert_within(o32[key], fx[gk], spread[key], key, float(np.abs(fx[gk] - o64[key]).max()))
    np.testing.assert_allclose(o32["ratio"], float(fx["info.ratio"]), rtol=1e-5)


def _offsets(n, net):
    from minimarl._lib import MappoDims, c_i64, lib
    offs = (c_i64 * 19)()
    d = MappoDims(3, 32, 5, n)
    rc = lib().mm_mappo_param_offsets(ctypes.byref(d), net, offs)
    return rc, list(offs), int(lib().mm_mappo_param_count(ctypes.byref(d), net))


@pytest.mark.parametrize("n", [0, 2])
def test_param_layout_and_scratch_counts_of_the_3_wide_shapes(n):
    """mm_mappo_param_offsets / _count at obs_dim 3: rows of W1 padded to 4 (critic over 2 agents: 6 -> 8), the
    Python views, and positive scratch counts of every gradient entry point."""
    from minimarl._lib import MappoDims, lib
    from minimarl.mappo import MappoNet
    H = 32
    for net, Din, Op in ((0, 3, 8), (1, 6 if n else 3, 4)):
        Dp = (Din + 3) // 4 * 4
        rc, offs, total = _offsets(n, net)
        sz = [Dp, Dp, H * Dp, H, H, H, H * H, H, H, H, 3 * H * H, 3 * H * H, 3 * H, 3 * H, H, H, Op * H, Op]
        assert rc == 0 and offs[:18] == [int(x) for x in np.cumsum([0] + sz[:-1])] and offs[18] == sum(sz) == total
        m = MappoNet(net, 3, 5, H, "cpu", cent_agents=n or None)
        assert m.total == total and tuple(m.view("W1").shape) == (H, Din) and tuple(m.view("ln0_w").shape) == (Din,)
    d = ctypes.byref(MappoDims(3, 32, 5, n))
    L_ = lib()
    # pass G's parked hiddens, d x2 of every row-step, the block partials of both passes (128 blocks per net and pass)
    pstride = (max(_offsets(n, 0)[2], _offsets(n, 1)[2]) + 3) // 4 * 4
    want = 2 * 128 * 4 * 2 * 5 * 1024 + 2 * 10 * 8 * 32 + 4 * 128 * pstride
    assert L_.mm_mappo_grad_scratch_count(d, 5, 10, 8) == want
    assert L_.mm_mappo_ff_grad_scratch_count(d) == 2 * 128 * pstride
    assert (L_.mm_mappo_wgrad_partial_count(d, 128) > 0) == (n == 0)   # the saves + wgrad path: decentralized only


def test_unbuilt_3_wide_shapes_are_refused_by_name():
    """(3, n) for n not in (1, 2): an error naming the built shapes, from the C ABI and from MappoPolicy."""
    from minimarl._lib import MappoDims, lib
    from minimarl.mappo import MappoPolicy
    for n in (3, 4):
        rc, _, total = _offsets(n, 1)
        msg = lib().mm_last_error().decode()
        assert rc != 0 and total < 0 and "unsupported dims" in msg and f"cent_agents={n}" in msg
        assert "cent_agents 2" in msg and "decentralized" in msg and f"critic input width {3 * n}" in msg
        assert lib().mm_mappo_grad_scratch_count(ctypes.byref(MappoDims(3, 32, 5, n)), 5, 10, 8) < 0
        assert lib().mm_mappo_ff_grad_scratch_count(ctypes.byref(MappoDims(3, 32, 5, n))) < 0
        with pytest.raises(RuntimeError, match=f"cent_agents={n}"):
            MappoPolicy(3, 5, 32, "cpu", cent_agents=n)
    assert _offsets(2, 1)[0] == 0 and lib().mm_mappo_param_count(ctypes.byref(MappoDims(6, 32, 5, 0)), 0) < 0


def test_config_env_switch():
    from minimarl.config import MappoTrainConfig, mappo_switch_reference
    assert MappoTrainConfig().env == "checkers"
    c = mappo_switch_reference()
    assert (c.env, c.n_agents, c.episode_length, c.recurrent) == ("switch", 2, 100, True)
    assert mappo_switch_reference(algorithm_name="mappo", use_centralized_V=True).recurrent is False
    with pytest.raises(ValueError, match="env="):
        MappoTrainConfig(env="Switch2-v0")
    with pytest.raises(ValueError, match="n_agents=4"):
        MappoTrainConfig(env="switch", n_agents=4, use_centralized_V=True)
    assert MappoTrainConfig(env="switch", n_agents=4).env == "switch"   # decentralized critic: any agent count


def test_policy_views_round_trip_the_golden_state():
    """MappoPolicy(3) loads and exports the reference-named state of both critic widths (host tensors only)."""
    from minimarl.mappo import MappoPolicy
    for name, (recurrent, cent) in sw.FWD_CASES.items():
        fx = sw.fwd_case(name)
        p = MappoPolicy(3, 5, 32, "cpu", cent_agents=2 if cent else None, recurrent=recurrent)
        p.actor.load_reference_state(fx, "actor.")
        p.critic.load_reference_state(fx, "critic.")
        assert (p.D, p.Dc) == (3, 6 if cent else 3)
        for net, kind in ((p.actor, "actor"), (p.critic, "critic")):
            for k, v in net.state_dict().items():
                np.testing.assert_array_equal(v.numpy(), fx[f"{kind}.{k}"])
            assert float(net.flat.abs().sum()) == pytest.approx(sum(float(np.abs(fx[f"{kind}.{k}"]).sum())
                                                                     for k in net.state_dict()), rel=1e-5)
