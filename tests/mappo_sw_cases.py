"""The Switch-width MAPPO fixtures (tests/golden/mappo_sw_*.npz, obs_dim 3, critic width 3 | 6) and the restatement's
runs on them, shared by tests/test_mappo_switch_cpu.py and tests/test_gpu_mappo_switch.py. A plain helper module (not
a conftest). The restatements are the existing ones, generic in the input width and used unchanged: oracle.mappo with
tests/mappo_mb_ref.py (recurrent nets, chunk minibatches; a centralized critic through tests/mappo_cv_ref.py) and
tests/mappo_ff_ref.py (feed-forward nets, row minibatches). Tolerances: tests/mappo_mb_ref.py's rule.

A train fixture holds cases; a case holds one synthetic rollout (data.*, before.*, vn0.*) and two reference runs on
it, m1 (train_batch_size 1) and m2 (train_batch_size 2, recorded permutations)."""
import functools
import os

import numpy as np
import torch

import mappo_cv_ref as cv
import mappo_ff_ref as ff
import mappo_mb_ref as mb
from oracle import mappo as om

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
D, A, H, N = 3, 5, 32, 2
# name -> (fixture, case, recurrent, centralized critic)
TRAIN_CASES = {"rec_d": ("mappo_sw_train", "d", True, False), "rec_c": ("mappo_sw_cv_train", "c", True, True),
               "ff_d": ("mappo_sw_ff_train", "d", False, False), "ff_c": ("mappo_sw_ff_train", "c", False, True)}
FWD_CASES = {"rec_d": (True, False), "rec_c": (True, True), "ff_d": (False, False), "ff_c": (False, True)}


@functools.lru_cache(maxsize=None)
def _npz(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def fwd_case(name):
    return cv.case(_npz("mappo_sw_fwd"), name)


def train_case(name, run):
    """The case's rollout and its run ``run`` ('m1' | 'm2') as one dict (the run's entries without their prefix)."""
    fixture, case, _, _ = TRAIN_CASES[name]
    c = cv.case(_npz(fixture), case)
    out = {k: v for k, v in c.items() if not k.startswith(("m1.", "m2."))}
    out.update(cv.case(c, run))
    return out


def keys(recurrent):
    return om.NET_KEYS if recurrent else ff.FF_KEYS


def nets(fx, recurrent, prefix=""):
    return cv.nets(fx, prefix) if recurrent else ff.nets(fx, prefix)


def share(obs_rows, E):
    """[E * N, 3] rows grouped by env -> the explicit cent_obs [E * N, 6]."""
    return torch.from_numpy(cv.share_obs(np.asarray(obs_rows).reshape(E, N, D)).reshape(E * N, N * D))


def fwd_oracle(fx, recurrent, cent):
    """(values, log-probs of the recorded actions, new actor hidden, new critic hidden) of a forward case; the
    feed-forward nets hand the hiddens back."""
    PA, PC = nets(fx, recurrent)
    t = lambda k: torch.from_numpy(fx[k])  # noqa: E731
    co = share(fx["obs"], int(fx["E"])) if cent else t("obs")
    if recurrent:
        return cv.get_actions_cv(PA, PC, t("obs"), co, t("ha")[:, 0], t("hc")[:, 0], t("masks"), t("actions"))
    v, _, lp = ff.get_actions(PA, PC, t("obs"), cent_obs=co if cent else None, actions=t("actions"))
    return v, lp, t("ha")[:, 0], t("hc")[:, 0]


def oracle_run(name, run, dtype, shuffle, perms="recorded", updates=None):
    """The restatement's train() of case ``name`` with the minibatches of run ``run``. perms: 'recorded' (the
    reference's permutations), or an array replacing them. -> (record per update, PA2, PC2, vn)."""
    _, _, recurrent, cent = TRAIN_CASES[name]
    fx = train_case(name, run)
    PA, PC = nets(fx, recurrent, "before.")
    data = {k[5:]: fx[k] for k in fx if k.startswith("data.")}
    vn0 = (float(fx["vn0.running_mean"][0]), float(fx["vn0.running_mean_sq"][0]), float(fx["vn0.debiasing_term"]))
    EP, M = int(fx["epochs"]), int(fx["train_batch_size"])
    pm = fx["perms"] if isinstance(perms, str) else perms
    if recurrent:
        return mb.ppo_train_mb(PA, PC, data, vn0, EP, int(fx["L"]), pm, M, dtype=dtype, shuffle=shuffle, cent=cent,
                               updates=updates)
    return ff.ppo_train_ff(PA, PC, data, vn0, EP, pm, M, dtype=dtype, shuffle=shuffle, cent=cent, updates=updates)


def outputs(name, rec, PA2, PC2, vn):
    out = (mb if TRAIN_CASES[name][2] else ff).train_outputs(rec, PA2, PC2, vn)
    out["norms"] = np.array([x for r in rec for x in (r["na"], r["nc"])])
    return out


def grads(name, rec, updates):
    return (mb if TRAIN_CASES[name][2] else ff).update_grads(rec, updates)


@functools.lru_cache(maxsize=None)
def oracle_case(name, run):
    """(fixture dict, (f64 train outputs, spreads), (f64 unclipped gradients of update 0, spreads), the outputs and
    gradients of the fp32 run in the reference's recorded order) of one case and run: the restatement's runs,
    computed once and read-only.

    The three runs behind a spread are the procedure's: m2 (minibatches: tests/mappo_mb_ref.py) fp32 on the recorded
    permutations, fp32 with every minibatch's members shuffled, f64; m1 (one full-batch update per epoch:
    tests/test_gpu_mappo.py's _fp32_spread) fp32 in the device's order -- the buffer's chunk / row order, which
    train() takes when it is given no permutation --, fp32 in a random order, f64. The recorded-order fp32 run of m1
    (the reference shuffles the single minibatch too) is what the CPU test pins to the golden."""
    fx = train_case(name, run)
    units = int(fx["perms"].shape[1])
    order = "recorded" if run == "m2" else np.arange(units)[None].repeat(int(fx["epochs"]), 0)
    runs = {}

    def r(dt, sh):
        if (dt, sh) not in runs:
            runs[(dt, sh)] = oracle_run(name, run, dt, sh, perms=order)
        return runs[(dt, sh)]

    train = mb.fp32_spread(lambda dt, sh: outputs(name, *r(dt, sh)))
    g = mb.fp32_spread(lambda dt, sh: grads(name, r(dt, sh)[0], (0,)))
    rec32 = r(torch.float32, False) if run == "m2" else oracle_run(name, run, torch.float32, False)
    return fx, train, g, outputs(name, *rec32), grads(name, rec32[0], (0,))
