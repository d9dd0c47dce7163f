"""CPU: the float64 / float32 restatement of tests/moffq_ref.py against the reference's own
M_QMix / M_VDN.train_policy_on_batch (fixtures tests/golden/moffq_*.npz, made by tests/golden/make_golden_moffq.py), the
case builder's fixed draws, and what the mm_moffq_* C ABI rejects before it launches anything (no device is touched)."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

from moffq_ref import AGENT_KEYS, CASES, GRID, TB, UNFILTERED, build_case, fixture_case

N8_K33_OBS_SHA256 = "be54784a2ef855decc3915f1956ef2dc64829fc79a5c80226e0d4aafb5a3a475"   # before the candidate filter came


@pytest.mark.parametrize("name", ["qmix", "vdn"])
def test_moffq_restatement_fp32_reproduces_reference(name):
    """Bit-equal on the CPU that recorded the fixtures (both variants pass there). rtol 1e-6 / atol 1e-7 is meant to
    leave room for another torch build's summation order, and for [qmix] it does not on every CPU: on the GPU host's CPU
    one element of 320 of the clipped Wo gradient (|g| = 7.1e-3, a cancelling sum over 38 rows of O(1) terms) came
    out 1.17e-7 off, against 1e-7 + 1e-6 |g| = 1.07e-7; everything else, and all of [vdn], passed there. With an earlier
    fixture seed the same host missed one element of 6016 of the updated hyper_w2.0.weight by 5.3e-7 (Adam's first
    step lr g / (|g| + eps) magnifies the noise of a near-zero g); make_golden_moffq.py now picks the seed against
    that. The bound is kept as set."""
    c, rec = fixture_case(name)
    r = c.r32
    tol = dict(rtol=1e-6, atol=1e-7)
    assert set(rec["grads"]) == set(r["clipped"]) == set(AGENT_KEYS) | set(c.M)
    for k in rec["grads"]:
        assert r["clipped"][k].dtype == torch.float32
        np.testing.assert_allclose(r["clipped"][k].numpy(), rec["grads"][k], err_msg="grad " + k, **tol)
        np.testing.assert_allclose(r["new"][k].numpy(), rec["new"][k], err_msg="post " + k, **tol)
    for k in ("loss", "grad_norm", "q_tot"):
        np.testing.assert_allclose(r[k], rec[k], err_msg=k, **tol)
    if c.use_per:
        np.testing.assert_allclose(r["prio"].numpy(), rec["prio"], err_msg="priorities", **tol)
    else:
        assert rec["prio"] is None and r["prio"] is None


@pytest.mark.parametrize("name", ["qmix", "vdn"])
def test_moffq_restatement_fp64_agrees_with_reference(name):
    """The float64 run against the recorded float32 arrays, at the r32-vs-r64 margins of the GPU file's preconditions."""
    c, rec = fixture_case(name)
    assert c.r64["grads"]["W1"].dtype == torch.float64
    for k in ("loss", "q_tot", "grad_norm"):
        np.testing.assert_allclose(rec[k], c.r64[k], rtol=5e-6, err_msg=k)
        np.testing.assert_allclose(c.r32[k], c.r64[k], rtol=5e-6, err_msg=k)
    if c.use_per:
        np.testing.assert_allclose(rec["prio"], c.r64["prio"].numpy(), rtol=5e-6)
    for k in rec["new"]:
        np.testing.assert_allclose(rec["new"][k], c.r64["new"][k].numpy(), rtol=1e-5, atol=2e-6, err_msg=k)


def test_moffq_fixture_preconditions():
    """What the fixtures are for: mixed dones_env, both Huber branches (VDN), an active clip (QMIX), the unused fc_h
    layer of the reference's MLPLayer in the state dict but neither trained nor mapped."""
    from minimarl.moffq import AGENT_REF
    for name in ("qmix", "vdn"):
        c, rec = fixture_case(name)
        assert (c.N, c.B, c.D) == (2, 19, 47)
        assert set(np.unique(c.batch["dones_env"])) == {0.0, 1.0}
        fc_h = [k for k in rec["files"] if "fc_h" in k]
        assert sorted(k for k in fc_h if k.startswith("q.")) == [f"q.mlp.mlp.fc_h.{i}.{p}" for i in (0, 2)
                                                                  for p in ("bias", "weight")]
        assert not [k for k in fc_h if k.startswith("grad.")]
        assert not [n for n in AGENT_REF.values() if "fc_h" in n]
        assert {"grad.q." + n for n in AGENT_REF.values()} == {k for k in rec["files"] if k.startswith("grad.q.")}
    c, rec = fixture_case("qmix")
    assert c.mixer == "qmix" and c.double_q and c.use_per and not c.huber and rec["grad_norm"] > c.max_norm
    c, rec = fixture_case("vdn")
    assert c.mixer == "vdn" and not c.double_q and not c.use_per and c.huber and not c.M
    assert 0.25 <= float((c.r64["err"].abs() > c.huber_delta).double().mean()) <= 0.75


def test_moffq_first_cases_draw_what_they_drew():
    """The candidate filter of the later cases left the first seven cases' inputs alone."""
    assert UNFILTERED == ("one_row", "tile_m1", "tile", "tile_p1", "blocks3", "d3_vdn", "n8_k33")
    assert hashlib.sha256(build_case("n8_k33").batch["obs"].tobytes()).hexdigest() == N8_K33_OBS_SHA256
    assert CASES["walk3_qmix"][1] == 2 * GRID + TB + 3 and GRID == 4096


# ---- rejections: every pointer that a kernel would read is null, so a launch would fault; none may happen
def dims(N=2, D=47, mixer=None, S=None, K=32, Hh=64):
    from minimarl._lib import MM_OFFQ_QMIX, OffqDims
    return OffqDims(N, D, 64, 5, MM_OFFQ_QMIX if mixer is None else mixer, N * D if S is None else S, K, Hh)


@pytest.mark.parametrize("kw,B", [(dict(), 0), (dict(), -1), (dict(K=65), 19), (dict(N=4097, D=3, K=1), 19),
                                  (dict(N=65, D=3, K=64), 19), (dict(D=48), 19)])
def test_moffq_workspace_bytes_rejects(kw, B):
    from minimarl._lib import lib
    assert lib().mm_moffq_workspace_bytes(ctypes.byref(dims(**kw)), B) == -1


def test_moffq_workspace_bytes_accepts_the_limits():
    from minimarl._lib import lib
    assert lib().mm_moffq_workspace_bytes(ctypes.byref(dims(N=64, D=3, K=64, Hh=8)), 1) > 0
    assert lib().mm_moffq_workspace_bytes(ctypes.byref(dims(N=4096, D=3, K=1)), 1) > 0


def test_moffq_loss_grad_rejects_before_launch():
    from minimarl._lib import MM_OFFQ_VDN, MoffqBatch, lib
    L, d = lib(), dims()
    need = int(L.mm_moffq_workspace_bytes(ctypes.byref(d), 19))
    assert need > 0
    one = ctypes.c_void_p(16)      # non-null, unmapped: reading it would fault

    def batch(**kw):
        bt = MoffqBatch()
        for k in ("obs", "nobs", "cent_obs", "cent_nobs", "acts", "rewards", "dones_env"):
            setattr(bt, k, one)
        bt.B, bt.double_q, bt.huber, bt.gamma, bt.huber_delta, bt.per_eps = 19, 1, 0, 0.99, 10.0, 1e-6
        for k, v in kw.items():
            setattr(bt, k, v)
        return bt

    call = lambda bt, P=one, PT=one, grad=one, ws=one, nbytes=need, stats=one, prio=one, dd=d: L.mm_moffq_loss_grad(
        ctypes.byref(dd), ctypes.byref(bt) if bt is not None else None, P, PT, grad, ws, nbytes, stats, prio, None)
    for kw in (dict(P=None), dict(PT=None), dict(grad=None), dict(ws=None), dict(stats=None)):
        assert call(batch(), **kw) == -22, kw
        assert b"null argument" in L.mm_last_error()
    assert call(None) == -22
    for k in ("obs", "nobs", "acts", "rewards", "dones_env"):
        assert call(batch(**{k: None})) == -22, k
    assert call(batch(), nbytes=need - 1) == -22 and b"workspace" in L.mm_last_error()
    assert call(batch(is_weight=one), prio=None) == -22 and b"priorities" in L.mm_last_error()
    assert call(batch(cent_obs=None)) == -22 and b"batch arrays" in L.mm_last_error()
    assert call(batch(cent_nobs=None)) == -22
    assert call(batch(B=0)) == -22
    assert call(batch(), dd=dims(K=65)) == -22 and b"mixer_hidden" in L.mm_last_error()
    # VDN needs no state: the same call without cent_obs gets past that check and stops at the short workspace
    dv = dims(mixer=MM_OFFQ_VDN)
    assert call(batch(cent_obs=None, cent_nobs=None), dd=dv, nbytes=0) == -22 and b"workspace" in L.mm_last_error()


def test_moffq_q_values_rejects_before_launch():
    from minimarl._lib import lib
    L, one = lib(), ctypes.c_void_p(16)
    q = lambda P=one, obs=one, out=one, R=4, d=None: L.mm_moffq_q_values(ctypes.byref(d or dims()), P, obs, None, out, R, None)
    assert q(R=0) == -22 and q(R=-1) == -22
    assert q(P=None) == -22 and q(obs=None) == -22 and q(out=None) == -22
    assert q(d=dims(D=48)) == -22
