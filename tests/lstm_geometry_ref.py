"""Case table and fp64 oracle for the BLSTM sweeps of csrc/lstm.hip OFF the headline's geometry: loaders that read HBM themselves
(flags bit 2, or more than 64 utterances) and staged sweeps with three or four batch groups.  A helper, not collected:
tests/test_lstm_geometry_ref_cpu.py holds the table and the oracle to their own properties (no GPU),
tests/test_lstm_geometry_gpu.py holds the kernels to the oracle.

The oracle of the LAYER (output, dx, the eight parameter gradients) is oracle/model_ref.blstm_layer_packed_equivalent in fp64 on
the fp32 parameters, with autograd.  The sweeps' own buffers (saved activations, c_t, d(pre-activations), bias partial sums) do
not come out of nn.LSTM, so ``sweep_steps`` restates one direction step by step in fp64 -- state held past an utterance's length,
outputs zero there, the reverse direction starting at each utterance's own last frame -- with the projection ``xproj`` as a
leaf: d(loss)/d(xproj) IS the gradient of the pre-activations.  The CPU file pins the restatement to the layer oracle.  Taking
xproj as an argument also lets the CPU file form what a sweep with a slot-reuse or clamp mistake would have written."""
import collections
import functools

import torch

from oracle import model_ref

HID = 256
IN_DIM = 512
GROUP = 16                       # utterances per cluster pair (G_CLUSTER's batch group)
FWD_LDS_RING, BWD_LDS_RING = 5, 6            # csrc/lstm.hip FWD_RING, BWD_RING: steps of xproj / saved rows in a workgroup's LDS
FWD_RING_STEPS, BWD_RING_STEPS = 16, 12      # .. and of the helpers' staging ring in the workspace
MAX_B = 128

# The bounds of check (a): tests/test_dense_lstm_gpu.py::test_blstm_layer_f32_mode_vs_torch_cpu, max-norm relative error
BOUND = {"f32": 1e-5, "bf16x3": 1e-3}

Case = collections.namedtuple("Case", "T B path lens idle why")
# path: "4" = flags bit 2 (no helper workgroups by flag), "helpers" = staged, 3+ groups, "NH" = no helpers by batch size (B > 64).
# idle: the group whose lengths are all <= 3 in the T = 37 cases (None elsewhere).
# Every group of two or more utterances holds one of length 1 and -- the idle group apart -- one of length T; a group of ONE
# utterance holds it at full length (it cannot hold both).
CASES = (
    # -- flags bit 2: the loaders read HBM themselves
    Case(1, 16, "4", [1] * 16, None,
         "no exchange at all; the loader's clamped look-ahead (s < T ? s : T - 1) runs past T from the first issue"),
    Case(2, 16, "4", [2, 1, 2, 2, 1, 2, 1, 1, 2, 2, 2, 1, 2, 1, 2, 2], None,
         "one exchange; look-ahead past T"),
    Case(5, 20, "4", [5, 3, 1, 4, 2, 5, 5, 3, 1, 4, 2, 2, 5, 4, 3, 1,   5, 1, 4, 3], None,
         "forward LDS ring (5) one short of reuse; backward (6) none; the second group holds 4 utterances"),
    Case(6, 20, "4", [6, 1, 5, 3, 4, 2, 6, 6, 1, 5, 2, 3, 4, 6, 5, 1,   3, 6, 1, 5], None,
         "forward LDS ring reuses one slot, backward ring exactly full"),
    Case(7, 20, "4", [7, 4, 1, 6, 2, 5, 3, 7, 7, 6, 1, 5, 2, 4, 3, 7,   6, 7, 1, 7], None,
         "both LDS rings reuse a slot"),
    Case(13, 16, "4", [13, 1, 12, 7, 9, 3, 13, 5, 11, 2, 8, 6, 10, 4, 13, 1], None,
         "one cluster pair; the small geometry of the changing-geometry sequence"),
    Case(13, 32, "4", [13, 7, 1, 10, 4, 12, 2, 9, 5, 13, 3, 8, 6, 11, 1, 12,   1, 13, 6, 11, 2, 9, 4, 7, 12, 3, 10, 5, 8, 13, 1, 6], None,
         "just past the backward staging ring (12): the same T as the staged case, for bit comparison with flags 0"),
    Case(17, 32, "4", [17, 1, 16, 9, 13, 5, 11, 3, 15, 7, 2, 12, 8, 14, 4, 17,   10, 17, 1, 6, 15, 3, 12, 8, 16, 2, 13, 5, 11, 7, 17, 1], None,
         "just past the forward staging ring (16)"),
    Case(37, 32, "4", [37, 1, 36, 19, 30, 7, 25, 12, 33, 4, 28, 15, 22, 9, 37, 2,   3, 1, 2, 3, 1, 1, 2, 3, 3, 2, 1, 1, 3, 2, 2, 3], 1,
         "every ring lapped at least twice, odd T (parity slots), ragged; the second group idles from step 3 on"),
    Case(200, 16, "4", [200, 199, 186, 173, 160, 147, 133, 120, 107, 94, 80, 67, 54, 40, 27, 1], None,
         "one longer chain on the path bench.py's shared-GPU mode uses; lengths from 200 down to 1"),
    # -- helpers on, three or four groups
    Case(13, 33, "helpers", [13, 1, 12, 6, 9, 3, 11, 5, 13, 2, 8, 7, 10, 4, 1, 12,   5, 13, 1, 9, 3, 11, 7, 2, 12, 6, 10, 4, 8, 13, 1, 11,   13], None,
         "the third group holds one utterance: a nearly empty cluster pair laps the backward staging ring"),
    Case(17, 33, "helpers", [17, 2, 15, 8, 12, 4, 10, 1, 16, 6, 13, 3, 9, 17, 5, 11,   1, 17, 7, 14, 2, 10, 5, 16, 8, 12, 3, 17, 6, 13, 1, 9,   17], None,
         "the same past the forward staging ring"),
    Case(37, 33, "helpers", [37, 1, 35, 18, 29, 6, 24, 11, 32, 3, 27, 14, 21, 8, 37, 16,   1, 3, 2, 1, 3, 3, 2, 1, 2, 3, 1, 2, 3, 1, 2, 3,   37], 1,
         "staging rings lapped twice and three times; the middle pair idles, the one-utterance pair runs to the end"),
    Case(37, 48, "helpers", [37, 5, 1, 31, 12, 26, 8, 37, 20, 3, 34, 15, 29, 10, 23, 1,   2, 1, 3, 3, 1, 2, 2, 3, 1, 3, 2, 1, 1, 2, 3, 3,   1, 37, 17, 36, 9, 28, 4, 22, 13, 33, 6, 25, 37, 19, 11, 30], 1,
         "six clusters"),
    Case(37, 64, "helpers", [37, 1, 33, 14, 27, 7, 21, 10, 35, 4, 30, 17, 24, 12, 37, 2,   9, 37, 1, 26, 13, 32, 5, 19, 36, 8, 23, 15, 29, 3, 37, 11,   3, 2, 1, 1, 2, 3, 3, 1, 2, 2, 3, 1, 1, 3, 2, 3,   37, 6, 28, 1, 18, 34, 10, 22, 37, 13, 31, 4, 25, 16, 1, 20], 2,
         "eight clusters: the last B with helpers"),
    # -- more than 64 utterances: no room for helpers
    Case(7, 65, "NH", [7, 1, 6, 3, 5, 2, 4, 7, 1, 6, 3, 5, 2, 4, 7, 1] * 4 + [7], None,
         "ten clusters; the fifth group holds one utterance: the batch clamp b = B - 1 is live in every DMA of that group"),
    Case(14, 65, "NH", [14, 1, 13, 6, 10, 3, 8, 14, 2, 12, 5, 9, 4, 11, 7, 1] * 4 + [14], None,
         "the same past both LDS rings twice"),
    Case(37, 65, "NH", [37, 1, 34, 16, 28, 5, 23, 11, 31, 3, 26, 13, 20, 8, 37, 18,   1, 37, 9, 30, 14, 35, 4, 21, 12, 27, 6, 33, 17, 24, 2, 37,
                        22, 7, 37, 1, 29, 15, 36, 10, 25, 3, 32, 19, 5, 27, 12, 37,   1, 2, 3, 3, 2, 1, 1, 3, 2, 3, 1, 2, 2, 1, 3, 3,   37], 3,
         "the same, every parity; the fourth pair idles beside four busy ones"),
    Case(14, 128, "NH", [14, 1, 13, 2, 12, 3, 11, 4, 10, 5, 9, 6, 8, 7, 14, 1] * 8, None,
         "the compiled-in limit: sixteen clusters, two per XCD, past both LDS rings twice"),
)
CASES = tuple(c._replace(lens=tuple(c.lens)) for c in CASES)      # hashable: the oracle is cached per case


def case_id(c):
    return f"T{c.T}-B{c.B}-{c.path}"


def case(T, B):
    (c,) = [c for c in CASES if (c.T, c.B) == (T, B)]
    return c


def native_flags(c):
    """The sweep flags a case is ABOUT (bit 2 for the "4" rows; the other paths are chosen by the batch size)."""
    return 4 if c.path == "4" else 0


SMALLEST = CASES[0]
# flags 0 against flags 4 wherever both exist (B <= 64); the write-through protocol (flags 1 and 5) on one case per family
BITWISE_CASES = tuple(c for c in CASES if c.B <= 64)
WRITE_THROUGH_CASES = (case(37, 32), case(37, 33))
# one workspace, changing geometry: (T, B, flags) in launch order
GEOMETRY_SEQUENCE = ((14, 128, 0), (13, 16, 4), (37, 33, 0), (14, 128, 0))


def groups(c):
    return [c.lens[i:i + GROUP] for i in range(0, c.B, GROUP)]


def make_inputs(c):
    """fp32 parameters in nn.LSTM's layout and initial distribution (U(-1/16, 1/16)), x, dy (zero past each length, like the
    gradient a packed reference hands back) and the lengths, all from one generator seeded by the shape."""
    g = torch.Generator().manual_seed(1000 * c.T + c.B)
    params = []
    for _ in range(2):
        for shape in ((4 * HID, IN_DIM), (4 * HID, HID), (4 * HID,), (4 * HID,)):
            params.append((torch.rand(shape, generator=g) * 2 - 1) / 16)
    x = torch.randn(c.T, c.B, IN_DIM, generator=g)
    dy = torch.randn(c.T, c.B, 2 * HID, generator=g)
    for b, n in enumerate(c.lens):
        dy[n:, b] = 0
    return params, x, dy, torch.tensor(c.lens, dtype=torch.int64)


def xproj(x, params, d):
    """(T,B,4H) fp64: x W_ih^T + b_ih + b_hh of direction d, torch's gate order i|f|g|o."""
    w_ih, _, b_ih, b_hh = params[4 * d:4 * d + 4]
    return x.double() @ w_ih.double().t() + (b_ih.double() + b_hh.double())


def sweep_steps(xp, w_hh, lens, reverse):
    """One direction, step by step, in xp's dtype: -> h (T,B,H) zero past each length, acts (T,B,4H) = sigma(i), sigma(f),
    tanh(g), sigma(o), zero past the length, c (T,B,H) = the cell state AFTER frame t's step (held where the utterance is over, so
    past the length it is the last state in the forward direction and 0 in the reverse one)."""
    T, B, _ = xp.shape
    lens = torch.as_tensor(lens)
    H = w_hh.shape[1]
    h = xp.new_zeros(B, H)
    c = xp.new_zeros(B, H)
    hs, acts, cs = [None] * T, [None] * T, [None] * T
    wt = w_hh.to(xp.dtype).t()
    for s in range(T):
        t = T - 1 - s if reverse else s
        pre = xp[t] + h @ wt
        i, f, g, o = pre.chunk(4, dim=1)
        i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
        cn = f * c + i * g
        hn = o * torch.tanh(cn)
        live = (t < lens)[:, None]
        c = torch.where(live, cn, c)
        h = torch.where(live, hn, h)
        hs[t] = torch.where(live, hn, torch.zeros_like(hn))
        acts[t] = torch.where(live, torch.cat([i, f, g, o], dim=1), xp.new_zeros(B, 4 * H))
        cs[t] = c
    return torch.stack(hs), torch.stack(acts), torch.stack(cs)


def gate_minor(a):
    """(T,B,4H) in torch's gate-major order -> (T,B,H,4), the sweeps' column order unit * 4 + gate."""
    T, B, _ = a.shape
    return a.reshape(T, B, 4, -1).permute(0, 1, 3, 2).contiguous()


def layer_outputs(xps, params, lens):
    """y (T,B,2H) from the two projections: what a pair of sweeps writes into ``out``."""
    return torch.cat([sweep_steps(xps[d], params[4 * d + 1], lens, bool(d))[0] for d in (0, 1)], dim=2)


@functools.lru_cache(maxsize=None)
def oracle(c):
    """Everything the checks compare with, in fp64, computed once per case and never modified:
    layer   y (T,B,2H), dx (T,B,I), grads (the eight parameter gradients, nn.LSTM's order)   -- blstm_layer_packed_equivalent
    sweeps  acts, dgates (T,B,2,H,4), c (T,B,2,H), dbias (2,H,4), dbias_group (groups,2,H,4) -- sweep_steps"""
    params, x, dy, lengths = make_inputs(c)
    p64 = [p.double().requires_grad_(True) for p in params]
    x64 = x.double().requires_grad_(True)
    y = model_ref.blstm_layer_packed_equivalent(x64.transpose(0, 1), lengths, p64).transpose(0, 1)
    y.backward(dy.double())
    o = {"y": y.detach(), "dx": x64.grad, "grads": [p.grad for p in p64]}
    acts, cs, dgs, ys = [], [], [], []
    for d in (0, 1):
        xp = xproj(x, params, d).requires_grad_(True)
        h, a, cc = sweep_steps(xp, params[4 * d + 1].double(), lengths, bool(d))
        (h * dy[:, :, d * HID:(d + 1) * HID].double()).sum().backward()
        ys.append(h.detach()); acts.append(gate_minor(a.detach())); cs.append(cc.detach()); dgs.append(gate_minor(xp.grad))
    o["y_steps"] = torch.cat(ys, dim=2)
    o["acts"] = torch.stack(acts, dim=2)
    o["c"] = torch.stack(cs, dim=2)
    o["dgates"] = torch.stack(dgs, dim=2)
    o["dbias"] = o["dgates"].sum(dim=(0, 1))
    o["dbias_group"] = torch.stack([o["dgates"][:, i:i + GROUP].sum(dim=(0, 1)) for i in range(0, c.B, GROUP)])
    return o


def rel_err(a, b):
    """Max-norm relative error (tests/pg_harness.rel_err on torch tensors)."""
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


# ------------------------------------------------------------------------------------------------------------------------
# what a sweep with a slot-reuse or clamp mistake would write (formed on the CPU only; nothing like it is ever built)
# ------------------------------------------------------------------------------------------------------------------------
def lapped_ring_outputs(c, group, lap=FWD_LDS_RING):
    """The layer output if, for ONE batch group, forward-sweep step s >= lap had read the xproj rows of step s - lap: a slot of the
    workgroups' LDS ring read one lap late.  Sweep step s is frame s (direction 0) or T - 1 - s (direction 1)."""
    params, x, _, lengths = make_inputs(c)
    rows = slice(group * GROUP, min(c.B, (group + 1) * GROUP))
    xps = []
    for d in (0, 1):
        xp = xproj(x, params, d)
        bad = xp.clone()
        for s in range(lap, c.T):
            t, t_old = (c.T - 1 - s, c.T - 1 - (s - lap)) if d else (s, s - lap)
            bad[t, rows] = xp[t_old, rows]
        xps.append(bad)
    return layer_outputs(xps, params, lengths)


def clamped_row_outputs(c, b):
    """The layer output if the loaders' batch clamp (b < B ? b : B - 1) had fired for the LIVE utterance b: its xproj rows are
    those of utterance B - 1."""
    params, x, _, lengths = make_inputs(c)
    xps = []
    for d in (0, 1):
        xp = xproj(x, params, d).clone()
        xp[:, b] = xp[:, c.B - 1]
        xps.append(xp)
    return layer_outputs(xps, params, lengths)
