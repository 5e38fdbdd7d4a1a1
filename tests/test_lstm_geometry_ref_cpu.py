"""tests/lstm_geometry_ref.py held to its own claims, without a GPU: the case table has the shapes and lengths it says it has, the
step-by-step restatement equals the layer oracle and torch's PackedSequence LSTM in fp64, and the bounds of the GPU checks are not
slack -- the output a sweep with a lapped LDS-ring slot or a misfired batch clamp would write misses them in both modes."""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import lstm_geometry_ref as R

NAMES = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
         "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse"]


def test_case_table_covers_the_paths_it_names():
    got = {(c.T, c.B, c.path) for c in R.CASES}
    want = ({(T, 16, "4") for T in (1, 2, 13, 200)} | {(T, 20, "4") for T in (5, 6, 7)} | {(T, 32, "4") for T in (13, 17, 37)}
            | {(T, 33, "helpers") for T in (13, 17, 37)} | {(37, 48, "helpers"), (37, 64, "helpers")}
            | {(T, 65, "NH") for T in (7, 14, 37)} | {(14, 128, "NH")})
    assert got == want and len(R.CASES) == len(want)
    for c in R.CASES:
        ngroups = (c.B + R.GROUP - 1) // R.GROUP
        # the path column says what lstm_launch does with the shape: helpers iff at most eight clusters and bit 2 clear
        assert (c.path == "NH") == (2 * ngroups > 8) and c.B <= R.MAX_B
        assert (c.path == "helpers") == (33 <= c.B <= 64)
        assert R.native_flags(c) == (4 if c.path == "4" else 0)
    # the rings each family is there to lap
    assert {c.T - R.FWD_LDS_RING for c in R.CASES if c.B == 20} == {0, 1, 2} and {c.T - R.BWD_LDS_RING for c in R.CASES if c.B == 20} == {-1, 0, 1}
    for B in (32, 33):
        Ts = sorted(c.T for c in R.CASES if c.B == B)
        assert Ts == [R.BWD_RING_STEPS + 1, R.FWD_RING_STEPS + 1, 37] and 37 > 2 * R.FWD_RING_STEPS and 37 % 2 == 1
    assert all(c.T >= 2 * R.BWD_LDS_RING + 2 for c in R.CASES if c.B in (128,)) and R.case(14, 65).T >= 2 * R.BWD_LDS_RING + 2
    assert all(c.B <= 64 for c in R.BITWISE_CASES) and {c.path for c in R.WRITE_THROUGH_CASES} == {"4", "helpers"}
    for T, B, flags in R.GEOMETRY_SEQUENCE:
        assert flags in (0, R.native_flags(R.case(T, B)))


@pytest.mark.parametrize("c", R.CASES, ids=R.case_id)
def test_case_lengths_have_the_stated_properties(c):
    assert len(c.lens) == c.B and all(1 <= n <= c.T for n in c.lens)
    gs = R.groups(c)
    assert len(gs) == (c.B + 15) // 16 and sum(len(g) for g in gs) == c.B
    assert (c.idle is not None) == (c.T == 37)
    for i, g in enumerate(gs):
        if len(g) == 1:
            assert g == (c.T,) and i != c.idle       # a group of one runs the whole sweep next to nothing
            continue
        assert 1 in g, (i, g)
        if i == c.idle:
            assert max(g) <= 3 and len(g) == R.GROUP     # a whole cluster pair idles through most of the sweep ..
        else:
            assert c.T in g, (i, g)
            if c.T > 2:
                assert len(set(g)) > 2, (i, g)       # .. and the others are ragged
    if c.idle is not None:
        assert sum(max(g) == c.T for g in gs) >= 1       # .. beside busy ones
    if c.B == 20:
        assert len(gs[1]) == 4
    if c.B in (33, 65):
        assert len(gs[-1]) == 1
    if (c.T, c.B) == (200, 16):
        assert list(c.lens) == sorted(c.lens, reverse=True) and c.lens[:2] == (200, 199) and c.lens[-1] == 1


def _packed_sequence_reference(c):
    params, x, dy, lengths = R.make_inputs(c)
    l64 = torch.nn.LSTM(R.IN_DIM, R.HID, 1, bidirectional=True).double()
    l64.load_state_dict({n: p.double() for n, p in zip(NAMES, params)})
    xr = x.double().requires_grad_(True)
    out, _ = l64(pack_padded_sequence(xr, lengths, enforce_sorted=False))
    out, _ = pad_packed_sequence(out, total_length=c.T)
    out.backward(dy.double())
    return out.detach(), xr.grad, [getattr(l64, n).grad for n in NAMES]


@pytest.mark.parametrize("c", [R.SMALLEST, R.case(7, 20)], ids=R.case_id)
def test_oracle_equals_packed_sequence_lstm_in_fp64(c):
    """The layer oracle against nn.LSTM on a PackedSequence, and the step-by-step restatement against both: output, dx, all eight
    parameter gradients; the bias gradient is the sum of d(pre-activations), by group as well."""
    o = R.oracle(c)
    y, dx, grads = _packed_sequence_reference(c)
    assert R.rel_err(o["y"], y) < 1e-13 and R.rel_err(o["dx"], dx) < 1e-12
    for n, a, b in zip(NAMES, o["grads"], grads):
        assert R.rel_err(a, b) < 1e-12, n
    assert R.rel_err(o["y_steps"], y) < 1e-13
    for d in (0, 1):
        db = o["dbias"][d].t().reshape(-1)          # (H,4) -> torch's gate-major 4H
        assert R.rel_err(db, grads[4 * d + 2]) < 1e-12 and R.rel_err(db, grads[4 * d + 3]) < 1e-12
    assert R.rel_err(o["dbias_group"].sum(0), o["dbias"]) < 1e-13
    # dW_hh from the restatement's own tensors: dgates_t^T h_prev(t), which ties dgates AND the saved h to the layer oracle
    T = c.T
    for d in (0, 1):
        dg = o["dgates"][:, :, d].permute(0, 1, 3, 2).reshape(T, c.B, -1)        # back to gate-major
        h = o["y_steps"][:, :, d * R.HID:(d + 1) * R.HID]
        want = torch.zeros(4 * R.HID, R.HID, dtype=torch.float64)
        if T > 1:
            a, b = (dg[1:], h[:-1]) if d == 0 else (dg[:-1], h[1:])
            want = a.reshape(-1, 4 * R.HID).t() @ b.reshape(-1, R.HID)
        assert float((want - grads[4 * d + 1]).abs().max()) <= 1e-12 * max(1.0, float(grads[4 * d + 1].abs().max()))


def test_oracle_is_silent_past_each_length():
    c = R.case(7, 20)
    o = R.oracle(c)
    for b, n in enumerate(c.lens):
        assert not o["y"][n:, b].any() and not o["acts"][n:, b].any() and not o["dgates"][n:, b].any()
        assert not o["c"][n:, b, 1].any()                                   # reverse direction: not started yet
        assert torch.equal(o["c"][n:, b, 0], o["c"][n - 1, b, 0].expand(c.T - n, -1))      # forward direction: held
        assert o["acts"][:n, b].abs().min() > 0


def test_a_lapped_lds_ring_slot_misses_the_bound_in_both_modes():
    """(7, 20): sweep steps 5 and 6 of the second group read the xproj rows of steps 0 and 1 -- the forward LDS ring (5 slots) one
    lap late.  The output error is far above the looser bound, so check (a) rejects it in "f32" and in "bf16x3"."""
    c = R.case(7, 20)
    assert c.T > R.FWD_LDS_RING and max(R.groups(c)[1]) == c.T
    e = R.rel_err(R.lapped_ring_outputs(c, group=1), R.oracle(c)["y"])
    print(f"[geometry] lapped LDS ring, (7, 20) group 1: output rel err {e:.2e}")
    assert e > 10 * max(R.BOUND.values()) and max(R.BOUND.values()) == R.BOUND["bf16x3"] > R.BOUND["f32"]
    # the first group's rows are untouched, and so are the frames of the steps before the lap
    bad, y = R.lapped_ring_outputs(c, group=1), R.oracle(c)["y"]
    assert R.rel_err(bad[:, :16], y[:, :16]) < 1e-13 and R.rel_err(bad[:R.FWD_LDS_RING, 16:, :R.HID], y[:R.FWD_LDS_RING, 16:, :R.HID]) < 1e-13


def test_a_misfired_batch_clamp_misses_the_bound_in_both_modes():
    """(7, 65): the clamp b = B - 1 applied to a live utterance of the fourth group (its rows replaced by utterance 64's)."""
    c = R.case(7, 65)
    b = 3 * R.GROUP + c.lens[3 * R.GROUP:].index(c.T)
    assert b < c.B - 1 and c.lens[b] == c.T
    bad, y = R.clamped_row_outputs(c, b), R.oracle(c)["y"]
    e = R.rel_err(bad, y)
    print(f"[geometry] misfired batch clamp, (7, 65) utterance {b}: output rel err {e:.2e}")
    assert e > 10 * max(R.BOUND.values())
    keep = [i for i in range(c.B) if i != b]
    assert R.rel_err(bad[:, keep], y[:, keep]) < 1e-13
