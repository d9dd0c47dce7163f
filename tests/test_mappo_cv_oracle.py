"""CPU: MAPPO with a centralized critic (use_centralized_V). The restatement (tests/mappo_cv_ref.py) against the
reference's golden vectors (tests/golden/mappo_cv_*.npz, share_obs derived from obs), at test_mappo_oracle.py's
tolerances, and the C ABI's parameter layout of the wide critic (host-only functions of libminimarl.so)."""
import ctypes

import numpy as np
import pytest
import torch

import mappo_cv_ref as cv
from oracle import mappo as om


@pytest.mark.parametrize("name", ["n2", "n8"])
def test_get_actions_and_values_golden(golden, name):
    fx = cv.case(golden("mappo_cv_fwd"), name)
    PA, PC = cv.nets(fx)
    E, N = int(fx["E"]), int(fx["N"])
    t = lambda k: torch.from_numpy(fx[k])
    cent = torch.from_numpy(cv.share_obs(fx["obs"].reshape(E, N, -1)).reshape(E * N, -1))
    v, lp, ha, hc = cv.get_actions_cv(PA, PC, t("obs"), cent, t("ha")[:, 0], t("hc")[:, 0], t("masks"), t("actions"))
    tol = dict(rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v.numpy(), fx["values"], **tol)
    np.testing.assert_allclose(v.numpy(), fx["values_only"], **tol)      # get_values on the same inputs
    np.testing.assert_allclose(lp.numpy(), fx["logp"], **tol)
    np.testing.assert_allclose(ha.numpy(), fx["ha_out"][:, 0], **tol)
    np.testing.assert_allclose(hc.numpy(), fx["hc_out"][:, 0], **tol)
    # the same share_obs for the agents of an env, yet distinct values: the critic hiddens differ per agent
    assert np.abs(np.diff(fx["values"].reshape(E, N), axis=1)).min() > 0


@pytest.mark.parametrize("name", ["n2", "n8"])
def test_evaluate_chunks_golden(golden, name):
    fx = cv.case(golden("mappo_cv_fwd"), name)
    PA, PC = cv.nets(fx)
    t = lambda k: torch.from_numpy(fx[k])
    L = int(fx["seq_L"])
    lp, ent = om.evaluate_chunks(PA, t("seq_obs"), t("seq_ha")[:, 0], t("seq_masks"), L, "actor", t("seq_actions"),
                                 t("seq_active"))
    v = om.evaluate_chunks(PC, t("seq_cent_obs"), t("seq_hc")[:, 0], t("seq_masks"), L, "critic")
    np.testing.assert_allclose(lp.numpy(), fx["seq_logp"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(v.numpy(), fx["seq_values"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(float(ent), float(fx["seq_entropy"]), rtol=1e-6)


@pytest.mark.parametrize("name,use_perm", [("n2", True), ("n2", False), ("n8", True), ("n8", False)])
def test_ppo_train_golden(golden, name, use_perm):
    fx = cv.case(golden("mappo_cv_train"), name)
    PA, PC, data, vn0, _ = cv.train_inputs(fx)
    E = int(fx["epochs"])
    rec, PA2, PC2, vn = cv.ppo_train_cv(PA, PC, data, vn0, E, int(fx["L"]), perms=fx["perms"] if use_perm else None)
    tol = dict(rtol=2e-4, atol=1e-7) if use_perm else dict(rtol=2e-3, atol=1e-6)
    for ep in range(E):
        for k in om.NET_KEYS:
            np.testing.assert_allclose(rec[ep]["ga"][k].numpy(), fx[f"grada{ep}.{om.ref_name(k, 'actor')}"],
                                       err_msg=f"actor {k} epoch {ep}", **tol)
            np.testing.assert_allclose(rec[ep]["gc"][k].numpy(), fx[f"gradc{ep}.{om.ref_name(k, 'critic')}"],
                                       err_msg=f"critic {k} epoch {ep}", **tol)
        np.testing.assert_allclose(rec[ep]["na"], fx["norms"][2 * ep], rtol=1e-5)
        np.testing.assert_allclose(rec[ep]["nc"], fx["norms"][2 * ep + 1], rtol=1e-5)
    if name != "n2":
        return   # (the N 8 case records gradients and norms only)
    for k in om.NET_KEYS:
        np.testing.assert_allclose(PA2[k].numpy(), fx[f"after.actor.{om.ref_name(k, 'actor')}"], rtol=1e-5, atol=2e-6)
        np.testing.assert_allclose(PC2[k].numpy(), fx[f"after.critic.{om.ref_name(k, 'critic')}"], rtol=1e-5,
                                   atol=2e-6)
    np.testing.assert_allclose(vn.m.numpy(), fx["vn1.running_mean"], rtol=1e-6)
    np.testing.assert_allclose(vn.msq.numpy(), fx["vn1.running_mean_sq"], rtol=1e-6)


def _offsets(D, n, net):
    from minimarl._lib import MappoDims, c_i64, lib
    offs = (c_i64 * 19)()
    d = MappoDims(D, 32, 5, n)
    rc = lib().mm_mappo_param_offsets(ctypes.byref(d), net, offs)
    return rc, list(offs), int(lib().mm_mappo_param_count(ctypes.byref(d), net))


@pytest.mark.parametrize("n", [2, 8])
def test_param_layout_of_the_wide_critic(n):
    """mm_mappo_param_offsets / _count with cent_agents: the critic's ln0 [Dc] and W1 [32, Dc] (rows padded to
    ceil4(Dc)), total = the sum of the padded tensors, the actor's layout unchanged."""
    D, H, Dc = 47, 32, 47 * n
    Dp = (Dc + 3) // 4 * 4
    rc, offs, total = _offsets(D, n, 1)
    assert rc == 0
    sz = [Dp, Dp, H * Dp, H, H, H, H * H, H, H, H, 3 * H * H, 3 * H * H, 3 * H, 3 * H, H, H, 4 * H, 4]
    assert offs[:18] == [int(x) for x in np.cumsum([0] + sz[:-1])]
    assert offs[18] == sum(sz) == total
    rc0, offs0, total0 = _offsets(D, n, 0)
    assert (rc0, offs0, total0) == _offsets(D, 0, 0)     # net 0 = the decentralized layout
    assert _offsets(D, 1, 1) == _offsets(D, 0, 1)        # cent_agents 1 = 0: the row's own obs
    # the Python views of the wide critic
    from minimarl.mappo import MappoNet
    net = MappoNet(1, D, 5, H, "cpu", cent_agents=n)
    assert net.total == total
    assert tuple(net.view("W1").shape) == (H, Dc) and tuple(net.view("ln0_w").shape) == (Dc,)
    assert tuple(net.view("ln0_b").shape) == (Dc,)
    assert tuple(MappoNet(0, D, 5, H, "cpu", cent_agents=n).view("W1").shape) == (H, D)


def test_param_layout_refuses_unsupported_cent_agents():
    from minimarl._lib import lib
    rc, _, total = _offsets(47, 3, 1)
    assert rc != 0 and total < 0
    msg = lib().mm_last_error().decode()
    assert "unsupported dims" in msg and "cent_agents=3" in msg
