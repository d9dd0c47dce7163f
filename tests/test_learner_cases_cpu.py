"""CPU: what the cases of tests/learner_cases.py are for holds before any device sees them. Per case: the kink and
argmax margins, the done placement (window cases: a done just before and just after every LDS window boundary and
one sample that crosses every boundary live), the Huber fraction, the clip state in float64, the exactly-zero
gradients of N = B = C = 1, the float32 oracle within 5e-6 (relative L2) of the float64 oracle for every gradient
tensor, and the dispatch facts that are pure functions of the shape, asked of the library's own host code
(mm_lrn_seq_windows, mm_mixer_fwd_seq_fits, mm_agent_mixer_pair_supported; no device is touched)."""
import ctypes
import os

import numpy as np
import pytest

from learner_cases import (CASES, MIN_KINK_MARGIN, MIN_TOP2_GAP, build_case, e32, grad_keys, huber_fraction_above,
                           window_boundaries)

# fp32 vs fp64 of the same arithmetic: 3e-8 .. 9.2e-7 measured per tensor at these shapes (C = 143 included)
GRAD_REL_L2 = 5e-6


def _lib():
    from minimarl._lib import LIB_PATH, lib
    if not os.path.exists(LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return lib()


@pytest.mark.parametrize("cid", list(CASES))
def test_learner_case_preconditions(cid):
    c = build_case(cid)
    assert c.kink_margin >= MIN_KINK_MARGIN and c.top2_gap >= MIN_TOP2_GAP
    dn = c.batch[4][:, :, 0].numpy()
    assert dn.shape == (c.B, c.C)
    assert (dn.sum(1) == 0).any()                       # a sample with no done at all
    if cid != "one":                                    # (its single entry is that sample)
        assert 0.03 <= dn.mean() <= 0.2, dn.mean()
        assert dn[:, :-1].any()                         # dones inside the chunks
    assert c.reset_mask.any() == c.reset_rows
    if c.reset_rows:
        st = c.batch[0]
        assert np.array_equal(c.reset_mask[:, 1:].numpy(), dn[:, :-1] > 0.5) and not c.reset_mask[:, 0].any()
        assert bool((st[c.reset_mask] == c.reset_obs).all())
    for kernel, bounds in window_boundaries(c).items():
        for s in bounds:
            assert dn[0, s - 1] == 1.0 and dn[1, s] == 1.0, (kernel, s)
            assert not dn[2, max(0, s - 2):s + 2].any(), (kernel, s)
    if c.mode == "qmix_min":
        assert 0.25 <= huber_fraction_above(c) <= 0.75, huber_fraction_above(c)
    if c.clip_state == "active":
        assert c.norm64[0] > 2 * c.clip
    if c.clip_state == "inactive":
        assert c.norm64[0] < 0.5 * c.clip
    g64 = c.o64["g"]
    if cid == "one":
        # zero hidden at the only step: the recurrent weights see no input. (The recurrent biases do get a gradient,
        # their n-gate rows included: d b_hh,n = d(n pre-activation) * r.)
        assert not g64["Whh"].any() and not g64["m.gWhh"].any()
        assert g64["bhh"][:, 64:].abs().min() > 0 and g64["m.gbhh"][64:].abs().min() > 0
    worst = 0.0
    for k in grad_keys(c):
        if not g64[k].any():
            assert not c.o32["g"][k].any(), k
            continue
        worst = max(worst, e32(c, k))
        assert e32(c, k) <= GRAD_REL_L2, (k, e32(c, k))
    print(f"{cid}: kink margin {c.kink_margin:.3g}, top-2 gap {c.top2_gap:.3g}, done rate {dn.mean():.3f}, "
          f"|g| {c.norm64[0]:.3g} / {c.norm64[1]:.3g} (clip {c.clip:g}), worst fp32-vs-fp64 rel L2 {worst:.3g}")


def test_learner_cases_cover_both_clip_states():
    states = {CASES[cid][12] for cid in CASES}
    assert {"active", "inactive"} <= states


@pytest.mark.parametrize("cid", list(CASES))
def test_learner_case_dispatch_facts(cid):
    """Window lengths, pairing and the mixer sequence fit as the launches' own host functions compute them, and the
    row / tile remainders the case is named for."""
    from minimarl._lib import QnetDims, c_i32
    L = _lib()
    c = build_case(cid)
    F1, G, H = c.agent
    d = QnetDims(c.N, c.D, F1, G, H, c.A)
    B, C, N, R = c.B, c.C, c.N, c.B * c.C
    Hm, K1 = c.mixer if c.mixer else (0, 0)
    rec = Hm in (32, 64)                # the mixer recurrence kernels exist for these
    out = (c_i32 * 3)()
    assert L.mm_lrn_seq_windows(ctypes.byref(d), Hm if rec else 0, C, out) == 0
    assert tuple(out) == (c.wins if c.wins else (C, C, C))
    if c.mixer:
        assert L.mm_mixer_fwd_seq_fits(B, N, Hm, K1) == c.fits
        assert L.mm_agent_mixer_pair_supported(ctypes.byref(d), B, C, N, N * c.D, Hm, K1) == c.pmask
        assert c.pair == (c.pmask == 3) and (not c.pair or c.split)
    if c.wins:
        wa, wb, wf = c.wins
        n_win = {"agent_bwd": -(-C // wa), "mixer_bwd": -(-C // wb), "mixer_fwd": -(-C // wf)}
        # (windows of the agent BPTT, the mixer backward, the mixer forward; steps of the ragged agent / mixer-backward
        # window, which those kernels run last, 0: none)
        expect = {"w13": (2, 1, 1, 6, 0), "w13_vdn": (2, 1, 1, 6, 0), "w49": (7, 2, 1, 0, 24), "w143": (16, 4, 2, 8, 35),
                  "w143_h32": (4, 2, 1, 35, 71)}[cid]
        assert (n_win["agent_bwd"], n_win["mixer_bwd"], n_win["mixer_fwd"], C % wa, C % wb) == expect
        if cid == "w143":
            assert C - wf == 71                    # the forward's second window
        bounds = window_boundaries(c)
        assert len(bounds["agent_bwd"]) == n_win["agent_bwd"] - 1
        if c.mixer:
            assert len(bounds.get("mixer_bwd", [])) == n_win["mixer_bwd"] - 1
            assert len(bounds.get("mixer_fwd", [])) == n_win["mixer_fwd"] - 1
    rem = {"t50_pair": (B % 4, B % 32, R, R % 8, R % 32), "t50_side": (B % 4, B % 32), "t50_vdn": (B % 4, c.D % 32),
           "t515": (B % 8, B % 32, R, R % 512, R % 64), "t1025_vdn": (B % 32, 2 * -(-B // 32) * N >= 512),
           "loss_b300": (R <= 1024, B > 256), "d64": (-(-c.D // 32),), "d65": (-(-c.D // 32),)}
    want = {"t50_pair": (2, 18, 350, 6, 30), "t50_side": (2, 18), "t50_vdn": (2, 1), "t515": (3, 3, 4120, 24, 24),
            "t1025_vdn": (1, True), "loss_b300": (True, True), "d64": (2,), "d65": (3,)}
    if cid in rem:
        assert rem[cid] == want[cid]
    if cid == "t515":
        assert 2 * -(-R // 32) * N > 2048          # past the row-block PRE's tile cap: the LDS PRE
    if cid == "t1025_vdn":
        assert 2 * -(-R // 32) * N <= 2048         # the row-block PRE


def test_seq_windows_query():
    """mm_lrn_seq_windows at the headline shape and at its first windowed chunk lengths; bad arguments."""
    from minimarl._lib import QnetDims, c_i32
    L = _lib()
    out = (c_i32 * 3)()
    d64, d32 = QnetDims(8, 47, 64, 64, 64, 5), QnetDims(8, 47, 64, 32, 32, 5)
    for d, Hm, C, want in ((d64, 64, 10, (10, 10, 10)), (d64, 64, 11, (11, 11, 11)), (d64, 64, 12, (6, 12, 12)),
                           (d64, 64, 48, (6, 48, 48)), (d64, 64, 49, (7, 25, 49)), (d64, 64, 141, (9, 36, 141)),
                           (d64, 64, 142, (9, 36, 71)), (d32, 32, 52, (52, 52, 52)), (d32, 32, 53, (27, 53, 53)),
                           (d32, 32, 129, (33, 129, 129)), (d32, 32, 130, (33, 65, 130)), (d64, 0, 142, (9, 142, 142))):
        assert L.mm_lrn_seq_windows(ctypes.byref(d), Hm, C, out) == 0
        assert tuple(out) == want, (Hm, C, tuple(out))
    assert L.mm_lrn_seq_windows(ctypes.byref(d64), 16, 10, out) == -22
    assert L.mm_lrn_seq_windows(ctypes.byref(d64), 64, 0, out) == -22
    assert L.mm_lrn_seq_windows(ctypes.byref(QnetDims(8, 47, 64, 64, 128, 5)), 0, 10, out) == -22


def test_mixer_bwd_fallback_rejects_hidden_above_its_scratch():
    """The fallback mixer backward kernels keep dhm0 [Hm] in the hypernet deltas' scratch [N*K1 + 3*K1]: a wider
    hidden is refused on the host, before any launch (the pointers are never dereferenced there)."""
    L = _lib()
    p = ctypes.c_void_p(64)
    B, N, S, Hm, K1 = 4, 1, 6, 64, 4           # N*K1 + 3*K1 = 16 < Hm
    assert L.mm_mixer_bwd(B, N, S, Hm, K1, p, p, p, p, p, p, p, p, None) == -22
    assert b"N*K1 + 3*K1" in L.mm_last_error()
    assert L.mm_mixer_bwd_seq(B, N, S, Hm, K1, p, p, p, p, p, p, p, p, p, None, 3, None) == -22
    assert b"N*K1 + 3*K1" in L.mm_last_error()
