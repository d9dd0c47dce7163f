"""Case builder shared by tests/test_learner_cases_cpu.py (CPU) and tests/test_gpu_learner_shapes.py (GPU): one
QLearner update (QMIX Train_dqn / VDN Target_Dqn / VDN Target_Double_Dqn / minimal QMIX) per case, the inputs plus
the CPU oracle's answer (oracle.nets.*_train_step) in float64 (the reference) and in float32 (the yardstick for
summation-order noise). Imports neither the library nor CUDA.

Inputs: parameters drawn as AgentQNet.init_default / Mixer.init_default draw them (U(+-1/sqrt(fan)) per tensor from
one seeded generator), a target net and mixer with their own seeds, a reference-shaped batch (states, actions,
rewards, next_states, dones, is_weight) and the env's reset observation [N, D]. Cases flagged reset_rows replace
states[b, t] by the reset observation wherever dones[b, t-1] is set (what the chunk store's gather does with an
offset of -1). Then the biases behind every non-smooth point of the behavior nets are moved by at most KINK_WINDOW
so that no row's argument lies within MIN_KINK_MARGIN of the kink (the two agent ReLU layers, the mixer's |.| on
w1 / w2, the ReLU on b2a, the mixing ReLU through b1b), and the Q-head biases of the target net (vdn_double: of the
behavior net too, whose copy is the double net) so that no top-2 Q gap is below MIN_TOP2_GAP. build_case asserts
the margins it reached.

Window cases (wins is set) place their dones: for every boundary between two LDS windows of every windowed kernel
sample 0 has a done at the step just before it, sample 1 at the step just after it, and sample 2 has no done at all
(so the carried dh / dhm / hidden crosses every boundary live); samples 0 and 1 get further dones away from the
boundaries, samples from 3 on draw theirs."""
import functools

import numpy as np
import torch

from oracle import nets

MIN_KINK_MARGIN = 1e-5    # float32 noise of these dot products is about 1e-6 (see tests/offq_cases.py)
MIN_TOP2_GAP = 1e-5
KINK_WINDOW = 2e-3        # the most a bias moves
GAMMA, LR = 0.99, 1e-3
DOUBLE_EPS = 0.3          # epsilon of the double net's eps-greedy draws (vdn_double)

AGENT_KEYS, MIXER_KEYS = nets.AGENT_KEYS, nets.MIXER_KEYS

# Per case: mode, agent (F1, G, H), mixer (Hm, K1) or None, N, D, A, B, C, then
#   reset_rows  states after a done inside the chunk are the reset observation (offset -1 on the device)
#   p_done      probability of the drawn dones
#   rew         reward scale (rewards = N(0, 1) * rew), clip = grad_clip; clip_state: what the float64 agent
#               gradient norm must be ("active": > 2 x clip, "inactive": < 0.5 x clip, None: not claimed)
#   wins        expected steps per LDS window (agent BPTT, mixer recurrence backward, mixer recurrence forward),
#               None where every sequence kernel runs a single window (then asserted to equal C)
#   split, pair QLearner._mixer_split() / _fwd_pair(); fits = mm_mixer_fwd_seq_fits; pmask =
#               mm_agent_mixer_pair_supported (None: no mixer)
# The launches each case takes (read from QLearner.compute_grads and the host dispatch in csrc/learner.hip,
# csrc/qmix_unit.hip, csrc/agent_fwd.hip) are listed in tests/test_gpu_learner_shapes.py.
_F = ("mode", "agent", "mixer", "N", "D", "A", "B", "C", "reset_rows", "p_done", "rew", "clip", "clip_state", "wins",
      "split", "pair", "fits", "pmask")
CASES = {
    "one":        ("qmix", (64, 32, 32), (32, 32), 1, 3, 2, 1, 1, False, 0.0, 1.0, 5.0, None, None, True, False, 1, 0),
    "t50_pair":   ("qmix", (64, 64, 64), (64, 32), 3, 47, 5, 50, 7, True, 0.12, 1.0, 5.0, None, None, True, True, 1, 3),
    "t50_side":   ("qmix", (64, 32, 32), (32, 32), 5, 47, 5, 50, 10, True, 0.1, 1.0, 0.5, "active", None, True, False,
                   1, 0),
    "t50_vdn":    ("vdn", (64, 32, 64), None, 3, 33, 5, 50, 10, True, 0.1, 1.0, 200.0, "inactive", None, False, False,
                   None, None),
    "t50_double": ("vdn_double", (64, 32, 32), None, 2, 47, 5, 50, 5, False, 0.1, 1.0, 5.0, None, None, False, False,
                   None, None),
    "t50_min":    ("qmix_min", (128, 32, 32), (64, 32), 4, 47, 5, 50, 6, False, 0.1, 0.75, 5.0, None, None, True,
                   False, 1, 0),
    "d64":        ("qmix", (64, 64, 64), (64, 32), 2, 64, 5, 33, 3, True, 0.12, 1.0, 5.0, None, None, True, True, 1, 3),
    "d65":        ("qmix", (64, 64, 64), (64, 32), 2, 65, 5, 33, 3, True, 0.12, 1.0, 5.0, None, None, True, False, 1,
                   2),
    "loss_b300":  ("vdn", (64, 32, 32), None, 2, 5, 5, 300, 3, False, 0.1, 1.0, 5.0, None, None, False, False, None,
                   None),
    "t515":       ("qmix", (64, 64, 64), (64, 32), 8, 11, 5, 515, 8, True, 0.1, 1.0, 5.0, None, None, False, False, 0,
                   0),
    "t1025_vdn":  ("vdn", (64, 32, 32), None, 8, 5, 5, 1025, 2, False, 0.1, 1.0, 5.0, None, None, False, False, None,
                   None),
    "w13":        ("qmix", (64, 64, 64), (64, 32), 2, 9, 5, 6, 13, False, 0.1, 1.0, 5.0, None, (7, 13, 13), True, True,
                   1, 3),
    "w13_vdn":    ("vdn", (64, 32, 64), None, 2, 9, 5, 6, 13, False, 0.1, 1.0, 5.0, None, (7, 13, 13), False, False,
                   None, None),
    "w49":        ("qmix", (64, 32, 64), (64, 32), 2, 9, 5, 5, 49, False, 0.1, 1.0, 5.0, None, (7, 25, 49), True, False,
                   1, 0),
    "w143":       ("qmix", (64, 64, 64), (64, 32), 2, 9, 5, 3, 143, False, 0.0, 1.0, 5.0, None, (9, 36, 72), True, True,
                   1, 3),
    "w143_h32":   ("qmix", (64, 32, 32), (32, 32), 2, 9, 5, 3, 143, False, 0.0, 1.0, 5.0, None, (36, 72, 143), True,
                   False, 1, 0),
    "m_k6":       ("qmix", (64, 32, 32), (32, 6), 3, 9, 5, 10, 5, False, 0.12, 1.0, 5.0, None, None, False, False, 1,
                   0),
    "m_h16":      ("qmix", (64, 32, 32), (16, 8), 3, 9, 5, 10, 5, False, 0.12, 1.0, 5.0, None, None, False, False, 0,
                   0),
    "m_h128":     ("qmix", (64, 32, 32), (128, 32), 8, 20, 5, 6, 5, False, 0.12, 1.0, 5.0, None, None, False, False, 0,
                   0),
}
# (behavior seed, target seed, batch seed) per case; a seed that misses a margin is replaced, never the margin
SEEDS = {cid: (11 + 10 * i, 12 + 10 * i, 13 + 10 * i) for i, cid in enumerate(CASES)}


def agent_shapes(N, D, A, F1, G, H):
    return {"W1": (N, F1, D), "b1": (N, F1), "W2": (N, G, F1), "b2": (N, G), "Wih": (N, 3 * H, G),
            "Whh": (N, 3 * H, H), "bih": (N, 3 * H), "bhh": (N, 3 * H), "Wq": (N, A, H), "bq": (N, A)}


def mixer_shapes(N, S, Hm, K1):
    return {"gWih": (3 * Hm, S), "gWhh": (3 * Hm, Hm), "gbih": (3 * Hm,), "gbhh": (3 * Hm,), "w1W": (N * K1, Hm),
            "w1b": (N * K1,), "w2W": (K1, Hm), "w2b": (K1,), "b1W": (K1, Hm), "b1b": (K1,), "b2aW": (K1, Hm),
            "b2ab": (K1,), "b2bW": (1, K1), "b2bb": (1,)}


def _draw(shapes, fan, seed):
    """One generator, the tensors in key order, each U(+-1/sqrt(fan)): what init_default writes into the flat buffer."""
    g = torch.Generator().manual_seed(int(seed))
    return {k: (torch.rand(int(np.prod(shp)), generator=g) * 2 - 1).mul(1.0 / np.sqrt(fan[k])).view(shp)
            for k, shp in shapes.items()}


def default_agent(seed, N, D, A, F1, G, H):
    fan = {"W1": D, "b1": D, "W2": F1, "b2": F1, "Wih": H, "Whh": H, "bih": H, "bhh": H, "Wq": H, "bq": H}
    return _draw(agent_shapes(N, D, A, F1, G, H), fan, seed)


def default_mixer(seed, N, S, Hm, K1):
    fan = {k: Hm for k in MIXER_KEYS}
    fan["b2bW"] = fan["b2bb"] = K1
    return _draw(mixer_shapes(N, S, Hm, K1), fan, seed)


def flat(P, keys):
    """The learner's flat parameter layout of a parameter dict."""
    return torch.cat([P[k].reshape(-1) for k in keys])


def window_boundaries(c):
    """First steps of the later LDS windows, per windowed kernel: the backward kernels walk windows of `win` steps
    down from C (for (w1 = C; w1 > 0; w1 -= win)), the forward recurrence up from 0."""
    if c.wins is None:
        return {}
    a, mb, mf = c.wins
    out = {"agent_bwd": [c.C - k * a for k in range(1, c.C) if c.C - k * a > 0]}
    if c.mixer:
        out["mixer_bwd"] = [c.C - k * mb for k in range(1, c.C) if c.C - k * mb > 0]
        out["mixer_fwd"] = [k * mf for k in range(1, c.C) if k * mf < c.C]
    return {k: v for k, v in out.items() if v}


def make_batch(c, seed):
    g = torch.Generator().manual_seed(int(seed))
    B, C, N, D, A = c.B, c.C, c.N, c.D, c.A
    st, ns = torch.rand(B, C, N, D, generator=g), torch.rand(B, C, N, D, generator=g)
    act = torch.randint(0, A, (B, C, N), generator=g).float()
    rew = torch.randn(B, C, N, generator=g) * c.rew
    dn = (torch.rand(B, C, 1, generator=g) < c.p_done).float()
    w = torch.rand(B, 1, generator=g) * 0.5 + 0.5
    reset_obs = torch.rand(N, D, generator=g)
    if c.wins is not None:
        dn[:3] = 0.0
        bounds = sorted({s for v in window_boundaries(c).values() for s in v})
        for s in bounds:
            dn[0, s - 1] = 1.0          # done at the step just before the boundary
            dn[1, s] = 1.0              # and just after it; sample 2 has none at all
        for t in range(5, C - 1, 11):   # further dones of samples 0 and 1, none within two steps of a boundary
            if all(t < s - 3 or t > s + 2 for s in bounds):
                dn[:2, t] = 1.0
    elif B > 1:
        dn[B - 1] = 0.0                 # one sample with no done at all
    mask = torch.zeros(B, C, dtype=torch.bool)
    if c.reset_rows:
        mask[:, 1:] = dn[:, :-1, 0] > 0.5
        st[mask] = reset_obs
    return (st, act, rew, ns, dn, w), reset_obs, mask


def center_bias(pre, bias):
    """Move each unit's bias by at most KINK_WINDOW so that 0 sits in the middle of the widest gap between that unit's
    arguments (pre [rows, units], float64, bias included) inside the window (as tests/offq_cases.py)."""
    pre = pre.reshape(-1, pre.shape[-1]).numpy()
    b = bias.double().numpy().copy()
    for j in range(b.shape[0]):
        v = pre[:, j]
        edges = np.concatenate([[-KINK_WINDOW], np.sort(v[np.abs(v) < KINK_WINDOW]), [KINK_WINDOW]])
        i = int(np.argmax(np.diff(edges)))
        b[j] -= 0.5 * (edges[i] + edges[i + 1])
    return torch.tensor(b, dtype=torch.float32)


def _q_seq(P, obs, dones):
    """Q of every (b, t, agent) in float64 with the chunk's hidden chain (zero at the start and after a done)."""
    B, C, N, _ = obs.shape
    P = {k: v.double() for k, v in P.items()}
    h = torch.zeros(B, N, P["Whh"].shape[2], dtype=torch.float64)
    out = []
    for t in range(C):
        q, nh = nets.agent_forward(P, obs[:, t].double(), h)
        out.append(q)
        h = nh * (1.0 - dones[:, t].double()).view(B, 1, 1)
    return torch.stack(out, 1)      # [B, C, N, A]


def kink_margin(c, adjust):
    """Smallest |argument| of the behavior nets' non-smooth points over the batch, in float64; adjust: centre the
    bias behind each of them first (center_bias), layer by layer, in c.P and c.M."""
    st, act, _, _, dn, _ = c.batch
    B, C, N, D = st.shape
    P, M, lo = c.P, c.M, []
    x = st.double().reshape(B * C, N, D)
    with torch.no_grad():
        for lay, (W, b) in enumerate((("W1", "b1"), ("W2", "b2"))):
            nxt = []
            for i in range(N):
                pre = x[:, i] @ P[W][i].double().t() + P[b][i].double()
                if adjust:
                    P[b][i] = center_bias(pre, P[b][i])
                    pre = x[:, i] @ P[W][i].double().t() + P[b][i].double()
                lo.append(float(pre.abs().min()))
                nxt.append(torch.relu(pre))
            x = torch.stack(nxt, 1)
        if not M:
            return min(lo)
        qa = _q_seq(P, st, dn).gather(3, act.long().unsqueeze(-1)).squeeze(-1)     # [B, C, N]
        Md = {k: v.double() for k, v in M.items()}
        hm, hs = torch.zeros(B, Md["gWhh"].shape[1], dtype=torch.float64), []
        for t in range(C):
            hm = nets.gru_cell(st[:, t].double().reshape(B, N * D), hm, Md["gWih"], Md["gWhh"], Md["gbih"], Md["gbhh"])
            hs.append(hm)
            hm = hm * (1.0 - dn[:, t].double()).view(B, 1)
        hs = torch.stack(hs, 1).reshape(B * C, -1)

        def layer(W, b, extra=0.0):
            pre = hs @ M[W].double().t() + M[b].double() + extra
            if adjust:
                M[b] = center_bias(pre, M[b])
                pre = hs @ M[W].double().t() + M[b].double() + extra
            lo.append(float(pre.abs().min()))
            return pre

        w1 = layer("w1W", "w1b").abs().view(B * C, -1, N)           # [rows, K1, N]
        layer("w2W", "w2b")
        layer("b2aW", "b2ab")
        layer("b1W", "b1b", torch.bmm(w1, qa.reshape(B * C, N, 1)).squeeze(-1))   # the mixing ReLU's argument
    return min(lo)


def top2_gap(P, obs, dones, adjust):
    """Smallest top-2 gap of the net's Q over the rows (float64); adjust: move P["bq"] first. An action's bias shifts
    its Q by the same amount in every row, so per agent and action the arguments to keep off 0 are Q_a - max of the
    other actions' Q."""
    with torch.no_grad():
        if adjust:
            for _ in range(2):
                q = _q_seq(P, obs, dones)
                N, A = q.shape[2], q.shape[3]
                for i in range(N):
                    qi = q[:, :, i].reshape(-1, A).clone()
                    for a in range(A):
                        others = torch.cat([qi[:, :a], qi[:, a + 1:]], 1).max(1)[0]
                        new = center_bias((qi[:, a] - others).unsqueeze(1), P["bq"][i, a:a + 1])
                        qi[:, a] += float(new[0]) - float(P["bq"][i, a])
                        P["bq"][i, a] = new[0]
        top = _q_seq(P, obs, dones).topk(2, dim=-1)[0]
    return float((top[..., 0] - top[..., 1]).min())


class Case:
    pass


def _to(x, dtype):
    if isinstance(x, dict):
        return {k: v.to(dtype) for k, v in x.items()}
    return tuple(v.to(dtype) for v in x)


def oracle_step(c, dtype):
    """oracle.nets.<mode>_train_step on the case in `dtype`: the oracle is dtype-agnostic apart from its torch.zeros,
    which follow the default dtype. Returns dict(P, M, g, loss, td); g holds the agent gradients after the clip and,
    under "m." + key, the mixer's (qmix: unclipped, qmix_min: after their own clip)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        P, T, M, TM, batch = _to(c.P, dtype), _to(c.PT, dtype), _to(c.M, dtype), _to(c.MT, dtype), _to(c.batch, dtype)
        out = {"M": {}, "td": None}
        if c.mode == "qmix":
            out["P"], out["M"], out["g"], out["loss"], out["td"] = nets.qmix_train_step(
                P, M, T, TM, batch, GAMMA, LR, c.clip, hidden_dim=c.mixer[1])
        elif c.mode == "qmix_min":
            out["P"], out["M"], out["g"], out["loss"] = nets.qmix_min_train_step(
                P, M, T, TM, batch, GAMMA, LR, grad_clip=c.clip, hidden_dim=c.mixer[1])
        elif c.mode == "vdn":
            out["P"], out["g"], out["loss"], out["td"] = nets.vdn_train_step(P, T, batch, GAMMA, LR, c.clip)
        else:
            out["P"], out["g"], out["loss"], out["td"] = nets.vdn_double_train_step(
                P, T, batch, GAMMA, LR, c.clip, DOUBLE_EPS, c.draws_u.to(dtype), c.draws_ra)
        return out
    finally:
        torch.set_default_dtype(old)


def raw_norms64(c):
    """The float64 gradient norms before any clip (agent tensors, mixer tensors): the oracle's loss + autograd."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        f64 = torch.float64
        P = {k: v.double().requires_grad_(True) for k, v in c.P.items()}
        M = {k: v.double().requires_grad_(True) for k, v in c.M.items()}
        T, TM, batch = _to(c.PT, f64), _to(c.MT, f64), _to(c.batch, f64)
        if c.mode == "qmix":
            loss = nets.qmix_loss(P, M, T, TM, batch, GAMMA, c.mixer[1])[0]
        elif c.mode == "qmix_min":
            loss = nets.qmix_min_loss(P, M, T, TM, batch, GAMMA, c.mixer[1])
        elif c.mode == "vdn":
            loss = nets.vdn_loss(P, T, batch, GAMMA)[0]
        else:
            loss = nets.vdn_double_loss(P, T, batch, GAMMA, DOUBLE_EPS, c.draws_u.double(), c.draws_ra)[0]
        ga = torch.autograd.grad(loss, [P[k] for k in AGENT_KEYS] + [M[k] for k in MIXER_KEYS if M])
        na = float(torch.sqrt(sum((g * g).sum() for g in ga[:len(AGENT_KEYS)])))
        nm = float(torch.sqrt(sum((g * g).sum() for g in ga[len(AGENT_KEYS):]))) if M else 0.0
        return na, nm
    finally:
        torch.set_default_dtype(old)


def min_errors64(c):
    """qmix_min: Q_tot - y of every (t, b) in float64, [C, B] (smooth-L1's argument; its kink is at |err| = 1)."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        f64 = torch.float64
        st, act, rew, ns, dn, w = _to(c.batch, f64)
        K1 = c.mixer[1]
        qtot = nets.qmix_qtot(_to(c.P, f64), _to(c.M, f64), (st, act, rew, ns, dn, w), K1)
        amax = _q_seq(c.PT, ns, dn).argmax(-1).double()
        tqtot = nets.qmix_qtot(_to(c.PT, f64), _to(c.MT, f64), (ns, amax, rew, ns, dn, w), K1)
        y = rew.sum(2).t() + GAMMA * tqtot * (1.0 - dn[:, :, 0].t())
        return qtot - y
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def build_case(cid):
    """Inputs and both oracle answers of one case (computed once per process; treat as read-only)."""
    c = Case()
    c.id = cid
    for k, v in zip(_F, CASES[cid]):
        setattr(c, k, v)
    ps, ts, bs = SEEDS[cid]
    F1, G, H = c.agent
    c.P, c.PT = default_agent(ps, c.N, c.D, c.A, F1, G, H), default_agent(ts, c.N, c.D, c.A, F1, G, H)
    c.M, c.MT = {}, {}
    if c.mixer:
        c.M = default_mixer(ps + 1000, c.N, c.N * c.D, *c.mixer)
        c.MT = default_mixer(ts + 1000, c.N, c.N * c.D, *c.mixer)
    c.batch, c.reset_obs, c.reset_mask = make_batch(c, bs)
    st, act, rew, ns, dn, w = c.batch
    assert not c.reset_rows or bool(c.reset_mask.any()), f"{cid}: no reset row"
    c.draws_u = c.draws_ra = None
    if c.mode == "vdn_double":
        g = torch.Generator().manual_seed(bs + 1)
        c.draws_u = torch.rand(c.C, c.B, generator=g)
        c.draws_ra = torch.randint(0, c.A, (c.C, c.B, c.N), generator=g)
    kink_margin(c, adjust=True)
    c.kink_margin = kink_margin(c, adjust=False)
    assert c.kink_margin >= MIN_KINK_MARGIN, f"{cid}: a ReLU / |.| argument of {c.kink_margin:.3g}"
    top2_gap(c.PT, ns, dn, adjust=True)
    c.top2_gap = top2_gap(c.PT, ns, dn, adjust=False)
    if c.mode == "vdn_double":      # the double net is a copy of the behavior net, run over s'
        top2_gap(c.P, ns, dn, adjust=True)
        c.top2_gap = min(c.top2_gap, top2_gap(c.P, ns, dn, adjust=False))
    assert c.top2_gap >= MIN_TOP2_GAP, f"{cid}: top-2 Q gap {c.top2_gap:.3g}; choose another seed"
    c.o64, c.o32 = oracle_step(c, torch.float64), oracle_step(c, torch.float32)
    assert c.o64["g"]["W1"].dtype == torch.float64 and c.o32["g"]["W1"].dtype == torch.float32
    c.norm64 = raw_norms64(c)
    if c.mode == "qmix_min":
        c.err64 = min_errors64(c)
        c.o64["td"] = c.err64[-1].abs()
    return c


def grad_keys(c):
    """Keys of the oracle's gradient dict: the 10 agent tensors, then the 14 mixer tensors ("m." + key)."""
    return list(AGENT_KEYS) + (["m." + k for k in MIXER_KEYS] if c.mixer else [])


def rel_l2(x, ref64):
    x, ref64 = np.asarray(x, np.float64), np.asarray(ref64, np.float64)
    return float(np.linalg.norm(x - ref64) / np.linalg.norm(ref64))


def e32(c, key):
    """The float32 oracle's relative L2 against the float64 oracle for one gradient tensor."""
    return rel_l2(c.o32["g"][key].numpy(), c.o64["g"][key].numpy())


def huber_fraction_above(c):
    """Fraction of the (t, b) entries whose float64 |err| lies above smooth-L1's delta of 1."""
    return float((c.err64.abs() > 1.0).double().mean())
