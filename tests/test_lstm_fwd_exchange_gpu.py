"""The f32-mode forward sweep's hand-off of h_t between the sixteen members of a cluster (csrc/lstm.hip, lstm_fwd_kernel<3>:
three bf16 planes per value, self-validating through their epoch-tagged LSBs).  Against the fp64 oracle at odd and even T,
ragged lengths, one and two batch groups; the same bits through the write-through publish path; the same bits from two sweeps
in a row on one workspace (prefill and parity tags tell stale words from fresh)."""
import numpy as np
import pytest
import torch

from oracle import model_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

NAMES = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
         "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse"]


def _rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / (np.abs(b).max() + 1e-30)


def _case(T, B, lens, seed):
    g = torch.Generator().manual_seed(seed)
    lstm = torch.nn.LSTM(512, 256, 1, bidirectional=True)
    x = torch.randn(T, B, 512, generator=g)
    return lstm, x, torch.tensor(lens, dtype=torch.int64)


def _forward(lstm, x, lengths, flags=0):
    from policy_gradient_asr_amd import functional as Fh, hipops
    hipops.LSTM_FLAGS = flags
    try:
        with hipops.precision("f32"), torch.no_grad():
            params = [getattr(lstm, n).detach().to(DEV) for n in NAMES]
            y = Fh.blstm_layer(x.to(DEV), lengths.to(torch.int32).to(DEV), params)
            torch.cuda.synchronize()
    finally:
        hipops.LSTM_FLAGS = 0
    hipops.lstm_assert_no_timeouts()
    return y.cpu()


@pytest.mark.parametrize("T,B,lens", [
    (201, 16, [201, 200, 199] + list(range(150, 20, -10))),          # odd T, ragged, one batch group
    (200, 32, [200] * 20 + list(range(199, 139, -5))),              # even T, ragged, two batch groups
    (1000, 32, [1000] * 16 + list(range(999, 499, -32))[:16]),       # the headline's chain length
    (3, 16, [3] * 8 + [2] * 4 + [1] * 4),                            # the first reads meet the prefill of both slots
])
def test_f32_forward_sweep_vs_fp64(T, B, lens):
    lstm, x, lengths = _case(T, B, lens, seed=3 * T + B)
    l64 = [getattr(lstm, n).detach().double() for n in NAMES]
    want = model_ref.blstm_layer_packed_equivalent(x.double().transpose(0, 1), lengths, l64).transpose(0, 1)
    y = _forward(lstm, x, lengths)
    err = _rel_err(y, want)
    print(f"[f32 forward sweep] T={T} B={B}: max rel err of the layer output vs fp64 {err:.2e}")
    assert err < 1e-5
    for b, n in enumerate(lens):
        assert torch.all(y[n:, b] == 0)


def test_f32_forward_write_through_same_bits():
    T, B, lens = 151, 32, [151] * 24 + list(range(150, 110, -5))
    lstm, x, lengths = _case(T, B, lens, seed=11)
    assert torch.equal(_forward(lstm, x, lengths, flags=0), _forward(lstm, x, lengths, flags=1))


@pytest.mark.parametrize("T", [97, 98])
def test_f32_forward_back_to_back_same_bits(T):
    """Two sweeps in a row on the cached workspace: the second starts on exchange slots that the first left full of
    fresh-looking words of both epochs, so only the per-call prefill keeps its first steps from taking them."""
    B, lens = 16, [T] * 12 + [T - 1, T - 2, 5, 1]
    lstm, x, lengths = _case(T, B, lens, seed=T)
    y0 = _forward(lstm, x, lengths)
    y1 = _forward(lstm, x, lengths)
    assert torch.equal(y0, y1)
