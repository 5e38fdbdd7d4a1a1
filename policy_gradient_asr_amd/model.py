"""Drop-in for the model-side names of the reference's model.py, running on the HIP kernels.

Kept names and positional signatures: ``weights``, ``nan_to_num``, ``Encoder``,
``Attention``, ``Decoder``, ``Seq2Seq``.  Documented divergences:
  * ``Encoder(n_feats=120)``: the reference hard-codes 120 MFCC features (model.py:37-38); the
    keyword makes the F=80 benchmark shape reachable while ``Encoder()`` is unchanged.
  * ``Seq2Seq.forward`` returns (T,B,V) log-probs from a CTC head ``nn.Linear(512, V)`` +
    log_softmax (the reference's Decoder prints a shape and returns None, model.py:117; the
    consumer contract is model.py:323).  ``Attention.forward`` / ``Decoder.forward`` (model.py:58-117) run
    as the reference executes them (pinned by its own outputs); a seq2seq TRAINING mode through them does not exist in
    the reference and is out of scope.
  * dropout (model.py:45,51 p=0.5; model.py:42 p=0.3) is applied only in train() mode like the
    reference; eval() is the parity mode.
"""
import torch
import torch.nn as nn

from . import functional as Fh
from . import hipops
from . import streams

HID = 256


def weights(m):
    """Xavier-normal on nn.Linear weights, bias 0.1 (model.py:19-25).  Used via model.apply."""
    if isinstance(m, nn.Linear):
        nn.init.xavier_normal_(m.weight.data)
        nn.init.constant_(m.bias.data, 0.1)


def nan_to_num(t, mynan=0.):
    """Non-finite entries -> mynan (model.py:27-32 does this recursively, element by element)."""
    if torch.all(torch.isfinite(t)):
        return t
    return torch.where(torch.isfinite(t), t, torch.as_tensor(mynan, dtype=t.dtype, device=t.device))


class Encoder(nn.Module):
    """InstanceNorm -> Linear(F,512)+leaky_relu(+dropout) -> 3-layer BLSTM(256) (model.py:34-56).

    Parameters carry the reference's state_dict names: input_layer.{weight,bias},
    blstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1,2}{,_reverse}."""

    def __init__(self, n_feats=120):
        super().__init__()
        self.n_feats = n_feats
        self.inst_norm = nn.InstanceNorm2d(n_feats)   # parameter-free; kept for state_dict/API parity
        self.input_layer = nn.Linear(n_feats, 512)
        self.blstm = nn.LSTM(input_size=512, hidden_size=HID, num_layers=3, dropout=0.3,
                             bidirectional=True, batch_first=True)
        self.drop = nn.Dropout()
        self.dropout_seed = 0x5EED          # masks are functions of (seed, call counter, index)
        self._drop_calls = 0

    def _layer_params(self, l):
        out = []
        for sfx in ("", "_reverse"):
            for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                out.append(getattr(self.blstm, f"{k}_l{l}{sfx}"))
        return out

    def forward_time_major(self, x, mask, lengths=None):
        """x (B,F,T), mask (B,T) -> (T,B,512) and int32 lengths (``lengths``: mask.sum(1) already on the device as int32)."""
        if not x.is_cuda:
            raise RuntimeError("policy_gradient_asr_amd.Encoder runs on the MI355X only (no CPU fallback)")
        if lengths is None:
            lengths = mask.sum(dim=1).to(torch.int32).contiguous()   # stays on the device: no host sync
        training = self.training
        # weight repacking (gate-permuted W_ih, its bf16 planes, the register-resident W_hh packs) depends on the
        # parameters only: all three layers' packs are made on a side stream while the front end runs
        packs = Fh.prepack_blstm_layers([self._layer_params(l) for l in range(3)], [512, 512, 512],
                                        rows=x.shape[0] * x.shape[2])
        # the affine's leaky'(y) factor is applied by whoever consumes y in the backward pass: the dropout that
        # follows it (train) or the first layer's input-gradient GEMM epilogue (eval)
        y = Fh.InstNormAffineFn.apply(x.float(), self.input_layer.weight, self.input_layer.bias, True)
        h = y
        if training:                                   # nn.Dropout(), model.py:45,51
            h = Fh.DropoutFn.apply(h, self.drop.p, self.dropout_seed, self._next_drop_offset(), True)
        for l in range(3):
            # nn.LSTM(dropout=0.3), model.py:42: the outputs of layers 0 and 1 are dropped on their way to the next layer --
            # by the sweep itself (its storer waves write h_t and dropout(h_t))
            od = (self.blstm.dropout, self.dropout_seed, self._next_drop_offset()) if (training and l < 2 and self.blstm.dropout > 0) else None
            h = Fh.blstm_layer(h, lengths, self._layer_params(l), dact_y=y if (l == 0 and not training) else None,
                               sweep_follows=(l > 0), prepacked=packs[l], out_dropout=od)
        return h, lengths

    def _next_drop_offset(self):
        self._drop_calls += 1
        return self._drop_calls

    def forward(self, x, mask):
        h, _ = self.forward_time_major(x, mask)
        return h.transpose(0, 1)   # (B,T,512) like model.py:56


class Attention(nn.Module):
    """model.py:58-94 as executed, on the MI355X (csrc/attention.hip, ``pgasr_attention_ctx``): per encoder frame the (H,H) outer
    product exp(d[r] e_i[k]) divided by its row sums lined up with the LAST axis (model.py:73's broadcast -- entry [r,k] by row k's
    sum; defect recorded in DESIGN.md), times the frame, summed over frames and over r.  dec_t (B,H), enc_out (B,T,H) -> (B,H).
    Forward only: the reference never trains through it (``Decoder.forward`` returns None, model.py:117)."""

    def __init__(self):
        super().__init__()

    def forward(self, dec_t, enc_out):
        from . import hipops
        return hipops.attention_ctx(dec_t.contiguous(), enc_out.contiguous())


class Decoder(nn.Module):
    """model.py:99-117: Decoder(alphabet_size, hidden_size) -- embedding(128) -> one-layer LSTM(128 -> hidden) -> per decoder step
    the attention context -> cat(dec_out[:, t], c_t).  Same parameter names / shapes as the reference (``embed_layer.weight``,
    ``lstm.*_l0``; ``nn.LSTM`` is a parameter container here, never called: its cuDNN/MIOpen path is not used).
    DOCUMENTED DIVERGENCE (like ``Seq2Seq.forward``): the reference builds the list `preds`, prints the shape of its stack and returns
    None (model.py:112-117); this returns that stack, (L, B, 2 * hidden), and prints nothing.  Forward only.
    The recurrent part is L dependent steps of (B,hidden) x (hidden,4 hidden) on the exact fp32 MFMA GEMM plus one cell kernel
    (``pgasr_lstm_cell_f32``) -- the BLSTM sweep kernels are built for H = 256 bidirectional layers and do not take this shape."""

    def __init__(self, alphabet_size, hidden_size):
        super().__init__()
        self.alphabet_size = alphabet_size
        self.hidden_size = hidden_size
        self.embed_layer = nn.Embedding(alphabet_size, 128)
        self.lstm = nn.LSTM(input_size=128, hidden_size=hidden_size, num_layers=1, batch_first=True)   # reference: dropout=0.3, a no-op with one layer
        self.attn = Attention()

    def forward(self, target_inputs, encoder_outputs, device=None):
        from . import hipops
        H = self.hidden_size
        w_ih, w_hh = self.lstm.weight_ih_l0.detach().contiguous(), self.lstm.weight_hh_l0.detach().contiguous()
        bias = (self.lstm.bias_ih_l0 + self.lstm.bias_hh_l0).detach().contiguous()
        if not w_ih.is_cuda:
            raise RuntimeError("Decoder.forward runs on the MI355X only (no CPU path)")
        B, L = target_inputs.shape
        x = self.embed_layer.weight.detach()[target_inputs.to(w_ih.device)].transpose(0, 1).contiguous()      # (L,B,128), time-major
        xp = torch.empty(L * B, 4 * H, dtype=torch.float32, device=w_ih.device)
        hipops.gemm(x.view(L * B, 128), w_ih, xp, M=L * B, N=4 * H, K=128, transB=True, bias=bias, precision=0)
        xp = xp.view(L, B, 4 * H)
        h = torch.zeros(B, H, dtype=torch.float32, device=w_ih.device)
        c = torch.zeros_like(h)
        g = torch.empty(B, 4 * H, dtype=torch.float32, device=w_ih.device)
        dec_out = torch.empty(L, B, H, dtype=torch.float32, device=w_ih.device)
        for t in range(L):
            hipops.gemm(h, w_hh, g, M=B, N=4 * H, K=H, transB=True, precision=0)
            hipops.lstm_cell(g, xp[t], c, h, dec_out[t])          # gates, c, h in one kernel (csrc/attention.hip)
        ctx = hipops.attention_ctx(dec_out, encoder_outputs.to(w_ih.device).contiguous())                       # (L,B,H): row q = t * B + b
        return torch.cat((dec_out, ctx), dim=2)


class Seq2Seq(nn.Module):
    """Seq2Seq(alphabet_size).forward(x, t, fmask, device) (model.py:174-183) with a CTC head."""

    def __init__(self, alphabet_size, n_feats=120):
        super().__init__()
        self.encoder = Encoder(n_feats=n_feats)
        self.head = nn.Linear(2 * HID, alphabet_size)

    def logits(self, x, fmask, lengths=None):
        """(T,B,V) pre-softmax scores and int32 lengths -- what the fused loss consumes."""
        h, lengths = self.encoder.forward_time_major(x, fmask, lengths)
        if hipops.head_logsoftmax_ok(self.head.in_features, self.head.out_features):
            # head + log-softmax in one kernel; the log-probs ride along for the fused loss (pg_ctc_loss takes them from the attribute)
            z, lp = Fh.HeadFn.apply(h, self.head.weight, self.head.bias)
            z.log_probs = lp
            z.log_probs_version = z._version      # an in-place edit of z afterwards (temperature, masking) invalidates lp: pg_ctc_loss checks
            return z, lengths
        return Fh.LinearFn.apply(h, self.head.weight, self.head.bias), lengths

    def forward(self, x, t, fmask, device=None):
        z, _ = self.logits(x, fmask)
        return Fh.LogSoftmaxFn.apply(z)        # differentiable log-probs for callers outside the fused loss


# ------------------------------------------------------------------------------------------
# driver shells: same positional signatures as model.py:186 / :277
# ------------------------------------------------------------------------------------------
def _read_alphabet(alphabet_path):
    with open(alphabet_path, "r") as fo:
        alphabet = ["<pad>"] + fo.readlines()                       # model.py:194-195
    char2ind = {alphabet[i].replace("\n", ""): i for i in range(len(alphabet))}   # model.py:197
    return alphabet, char2ind


def _to_device(batch, device):
    x = batch["feat"].to(device)                                    # model.py:227-230
    t = batch["trans"].to(device)
    fmask = batch["fmask"].squeeze(1).to(device)
    tmask = batch["tmask"].squeeze(1).to(device)
    return x, t, fmask, tmask


FEATURE_DIMS = {"mfcc": 120, "logmel80": 80}      # what data.collate_custom(features=...) produces from a waveform


def _check_features(features, n_feats, dataset, stack=1):
    """A waveform-carrying dataset meets the model through the front end: its width must be the model's n_feats (a mismatch
    used to surface as a shape error at the instance norm of the first step).  stack: the frames a ``FrameStack`` policy stacks
    between the two -- the model's width is then FEATURE_DIMS[features] * stack."""
    if features not in FEATURE_DIMS:
        raise ValueError(f"features must be one of {sorted(FEATURE_DIMS)}")
    try:
        item = dataset[0] if dataset is not None and len(dataset) > 0 else None
    except Exception:
        item = None
    if isinstance(item, dict) and ("wave" in item or "aud" in item) and "feat" not in item:
        if n_feats != FEATURE_DIMS[features] * stack:
            raise ValueError(f"features='{features}' gives {FEATURE_DIMS[features]} features per frame but n_feats={n_feats}" if stack == 1 else
                             f"features='{features}' stacked {stack} times gives {FEATURE_DIMS[features] * stack} features per frame "
                             f"but the model takes {n_feats}")


def _frame_stack_of(model_path, frame_stack, who):
    """The low-frame-rate policy ``predict`` / ``align`` run with: the one <model_path>/checkpoint_last.pth was trained with, which a
    given ``frame_stack`` must agree with (ValueError); without a checkpoint, or with one that has no such field, the argument."""
    import os
    from .features import FrameStack
    frame_stack = FrameStack.coerce(frame_stack)
    ckpt = os.path.join(model_path, "checkpoint_last.pth")
    if not os.path.exists(ckpt):
        return frame_stack
    st = torch.load(ckpt, map_location="cpu")
    if "frame_stack" not in st:
        return frame_stack
    saved = FrameStack.coerce(st["frame_stack"])
    if frame_stack is not None and frame_stack != saved:
        raise ValueError(f"{who}: frame_stack={frame_stack!r} but the model in {model_path} was trained with frame_stack={saved!r}")
    return saved


def _read_wav_dir(path):
    """Every *.wav of a directory, in sorted order -> (waveforms, sample rates)."""
    import os
    from .features import read_wav
    names = sorted(f for f in os.listdir(path) if f.lower().endswith(".wav"))
    if not names:
        raise ValueError(f"{path}: no .wav files")
    waves, rates = [], []
    for f in names:
        try:
            import torchaudio
            w, sr = torchaudio.load(os.path.join(path, f))
            w = w[0]
        except ImportError:
            w, sr = read_wav(os.path.join(path, f))
        waves.append(w)
        rates.append(int(sr))
    return waves, rates


def _wave_augment(noise_dir, rir_dir, snr_db, noise_prob, rir_prob, device):
    """None where both directories are None, else the features.WaveAugment over their files."""
    if noise_dir is None and rir_dir is None:
        return None
    from .features import NoiseBank, RirBank, WaveAugment
    noise = None if noise_dir is None else NoiseBank(*_read_wav_dir(noise_dir), device=device)
    rir = None if rir_dir is None else RirBank(*_read_wav_dir(rir_dir), device=device)
    return WaveAugment(noise=noise, snr_db=snr_db, noise_prob=noise_prob, rir=rir, rir_prob=rir_prob)


def train(corpus_path, model_path, num_epochs, batch_size, device, train_dataset=None, dev_dataset=None,
          n_feats=120, lam=1.0, lr=5e-4, resume=True, log_every=10, seed=0, bucket_by_length=True, features="mfcc",
          precision="f32", num_samples=1, reward_baseline="hypothesis", reward_unit="char", max_grad_norm=None,
          accumulate_steps=1, score_function="path", max_hyp_len=None, entropy_weight=0.0, objective="reinforce", mwer_nbest=4,
          mwer_beam=16, init_from=None, kl_weight=0.0, kl_reference_path=None, mwer_lm_path=None, mwer_lm_alpha=0.0,
          mwer_lm_beta=0.0, target_rate=None, speed_perturb=None, noise_dir=None, rir_dir=None, snr_db=(5.0, 20.0), noise_prob=1.0,
          rir_prob=0.5, units_path=None, wide_alphabet=None, wide_objectives=None, wide_sequence=None,
          mwer_unit_lm_path=None, spelled_reward=False, reward_mode="utterance", step_objectives=None, frame_stack=None):
    """Epoch loop of model.py:186-274 on the MI355X path: per-epoch train loss -> train_loss.npy,
    validation CTC loss -> val_losses.npy, model_best.pth / model_last.pth (state_dicts, reference
    names), plus checkpoint_last.pth (model + Adam moments + epoch) from which ``resume`` restarts
    -- the reference saves weights only.  ``train_dataset`` / ``dev_dataset`` default to the
    reference's Data(train.tsv / dev.tsv, clips) and accept any Dataset of collate_custom items.
    features: "mfcc" (the reference's 120 MFCC + delta features, n_feats=120) or "logmel80" (80-band log-mel, n_feats=80) for
    items that carry waveforms / audio paths; the collate function leaves the features on the GPU (data.collate_custom(device=...)):
    from the front end to the trainer they never visit the host.
    precision: "f32" (default: the reference's torch-fp32 arithmetic, model.py:38-44) or "bf16x3" (opt-in, ~20 % faster,
    within 1e-3 on loss and gradients) -- hipops.PRECISION_MODES.
    num_samples / reward_baseline: sampled paths per utterance and the baseline their rewards are scored against ("hypothesis":
    the greedy path's reward; "leave_one_out": the mean reward of the other samples, num_samples >= 2) -- PolicyGradientTrainer.
    reward_unit: "char" (default) or "word" -- the word-level reward -WED / W(y), words split at the alphabet's " " symbol (which
    alphabet.txt must then hold).
    score_function: "path" (default) or "sequence" -- score every sample by the CTC likelihood of its collapsed hypothesis instead of
    its frame path (same expected gradient, lower variance); max_hyp_len caps the hypotheses so scored (None: every one of at most
    min(T, 1023) tokens; longer ones keep the path-level term) and with it the lattice workspace -- PolicyGradientTrainer.
    entropy_weight: 0 (default: off) or beta > 0 -- entropy regularisation of the frame policy against collapse: the loss gains
    -beta / batch times every utterance's MEAN frame entropy (nats), so beta is in loss units per nat per frame and does not grow with
    T -- PolicyGradientTrainer.  The log lines then carry the batch-mean entropy.
    init_from: None (default) or the path of a state dict (a ``model_best.pth``, e.g. of a lam=0 CTC run) that the model starts from:
    loaded after the ``weights`` init when no resume checkpoint is found -- the second stage of the two-stage recipe, CTC pretraining
    followed by a policy-gradient fine-tune.
    kl_weight: 0 (default: off) or gamma > 0 -- a KL penalty that anchors the fine-tune to a frozen reference policy: the loss gains
    gamma / batch times every utterance's MEAN frame KL(policy || reference) in nats -- PolicyGradientTrainer.  The reference is a
    second model loaded from ``kl_reference_path`` (default: ``init_from``; one of the two is required), also in a resumed run: never
    from the checkpointed model, which has moved.  The log lines then carry the batch-mean KL.  Not with objective="mwer".
    max_grad_norm: None (default) or a bound > 0 on the global L2 norm of a step's gradient, clipped on the device inside the step
    (clip_grad_norm_ between backward and the update; a step whose gradient holds an inf / NaN is skipped) -- PolicyGradientTrainer.
    The log lines then carry the last gradient norm, and the end of an epoch the counts of clipped and skipped steps.
    accumulate_steps: 1 (default: one optimizer step per loader batch, as always) or n > 1 -- n consecutive loader batches are the
    micro-batches of ONE optimizer step (PolicyGradientTrainer.step_accumulated: the batch of an update is n x batch_size; the last
    group of an epoch may be shorter).  The log lines and the epoch mean then count optimizer steps.  Each loader batch keeps its
    own padded length, so the update is that of the n batches' summed loss, not of one batch padded to a common length.
    objective: "reinforce" (default: the sampled objectives above, today's trainer with today's arguments) or "mwer" -- MWER over the
    ``mwer_nbest`` best hypotheses of the width-``mwer_beam`` beam search (mwer.MWERTrainer: nothing is sampled, so num_samples,
    reward_baseline, score_function and entropy_weight must keep their defaults; reward_unit chooses the char or word risk and
    max_hyp_len caps the hypotheses in the list's posterior).
    mwer_lm_path: None (default) or an ``lm.npz`` of ``build_lm``: with objective="mwer" the N-best lists come from the search fused
    with that LM at weights mwer_lm_alpha / mwer_lm_beta (the ones ``predict(lm_path=, lm_alpha=, lm_beta=)`` will decode with), on the
    single-wave kernel; the posterior over the list stays the exact CTC likelihood -- mwer.MWERTrainer.
    target_rate: None (default: every waveform is taken to be at 16 kHz whatever its file says, as in the reference) or 16000: audio
    at another rate (Common Voice clips are 48 or 32 kHz) is converted on the device in front of the framing (features.Resample);
    validation batches too.
    speed_perturb: None (default) or a features.SpeedPerturb (or its factors, e.g. (0.9, 1.0, 1.1)): every training waveform is
    resampled by a factor drawn per (seed, epoch, utterance index) -- the dataset is then wrapped in data.Indexed, and the draws
    change every epoch.  The length bucketing keeps using the UNPERTURBED lengths: a batch's utterances differ by at most the
    extreme factors' ratio more than they would.  Validation is not perturbed.
    noise_dir / rir_dir: None (default) or a directory of WAV files (read with torchaudio where present, else features.read_wav):
    noise recordings and room impulse responses, packed on the device once at 16 kHz (features.NoiseBank / RirBank).  Every training
    waveform then takes noise with probability noise_prob at an SNR drawn uniformly from snr_db = (low, high) dB, and a reverberation
    with probability rir_prob (features.WaveAugment), drawn per (seed, epoch, utterance index) behind the resampling and in front of
    the framing.  Validation and ``predict`` are never augmented.
    units_path: None (default: <corpus_path>/alphabet.txt, one character per symbol) or a units file of ``build_units`` /
    ``units.SubwordUnits.save`` that stands in its place: the transcripts are encoded by greedy longest match over the units, the
    output layer has one symbol per unit (and the blank), and the reward is the edit distance over units.
    wide_alphabet: None (default: "more than 64 symbols") or a bool -- PolicyGradientTrainer(wide_alphabet=): up to 1024 symbols with
    the default objective (num_samples=1, the greedy baseline, reward_unit="char", score_function="path", no entropy or KL term);
    objective="mwer" does not take it.
    wide_objectives: None / False (default: the line above) or True -- PolicyGradientTrainer(wide_objectives=True): with more than
    64 symbols num_samples 1..16, either reward_baseline, entropy_weight and kl_weight (with init_from / kl_reference_path) run on
    the wide kernels too; the word reward and score_function="sequence" stay refused there.  Needs wide_alphabet; kept in the
    checkpoint beside it.
    reward_mode: "utterance" (default: one reward per utterance) or "per_step" -- the reward-to-go of every frame in the REINFORCE
    term (PolicyGradientTrainer(reward_mode=)); alone it takes num_samples=1 with the hypothesis baseline and at most 64 symbols;
    objective="mwer" does not take it.
    step_objectives: None / False (default) or True -- PolicyGradientTrainer(step_objectives=True): reward_mode="per_step" then runs
    with num_samples 1..16, either reward_baseline, entropy_weight and kl_weight, and with wide_alphabet (above 64 symbols K > 1, leave
    one out, entropy and KL need wide_objectives as well).  Kept in the checkpoint beside wide_objectives and checked on resume.
    wide_sequence: None (default: False, or what the checkpoint of a resumed run holds) or a bool -- with more than 64 symbols,
    objective="mwer" (mwer_nbest <= 16, mwer_beam <= 128, reward_unit="char"; mwer.MWERTrainer(wide_sequence=True)) and
    score_function="sequence" (PolicyGradientTrainer(wide_sequence=True)) run on the wide kernels too.  Set max_hyp_len for unit
    models: the hypothesis lattices take 2 * K*B*T * roundup64(2*Lh+1) * 4 bytes.  Needs wide_alphabet; kept in the checkpoint beside it.
    mwer_unit_lm_path: None or a ``lm.UnitNgramLM.save`` file: with objective="mwer" and wide_sequence the lists come from the wide
    search fused with that unit LM at weights mwer_lm_alpha / mwer_lm_beta.
    spelled_reward: False (default: the line under units_path -- the reward is the edit distance over units) or True, with
    units_path: the rewards (the risk of objective="mwer") are counted on the SPELLED text of targets and hypotheses -- reward_unit=
    "char" its characters, "word" its words, the metrics that are reported -- through a ``units.UnitSpelling`` built from the units
    file and <corpus_path>/alphabet.txt (PolicyGradientTrainer(unit_spelling=), mwer.MWERTrainer(unit_spelling=)); above 64 symbols it
    is what admits reward_unit="word".  Kept in the checkpoint beside wide_alphabet.
    frame_stack: None (default: every frame of the front end is one step of the sweeps) or (stack, skip[, left]) / a
    features.FrameStack -- low-frame-rate input: every batch, training and validation, is stacked and subsampled on the device behind
    the front end and its augmentation (data.collate_custom(frame_stack=)), the model is built with n_feats * stack inputs (n_feats
    stays the front end's width) and sees ceil(n / skip) frames per utterance.  An utterance whose transcript no longer fits its
    frames (features.FrameStack.fits) gets zero weight from the loss as ever; they are counted on the device and printed once per
    epoch.  Kept in the checkpoint beside wide_alphabet, where ``predict`` and ``align`` find it; a resume with another policy is
    refused."""
    import os
    import numpy as np
    import torch.utils.data as tud
    import functools
    from .data import Data, LengthBucketSampler, dataset_lengths
    from .data import collate_custom as _collate
    from .loss import pg_ctc_loss
    from .train_step import PolicyGradientTrainer

    if isinstance(accumulate_steps, bool) or int(accumulate_steps) != accumulate_steps or accumulate_steps < 1:
        raise ValueError(f"accumulate_steps must be an integer >= 1 (got {accumulate_steps!r})")
    accumulate_steps = int(accumulate_steps)
    if objective not in ("reinforce", "mwer"):
        raise ValueError(f"objective must be 'reinforce' or 'mwer' (got {objective!r})")
    from .loss import check_kl_weight
    kl_weight = check_kl_weight(kl_weight)
    if kl_reference_path is None:
        kl_reference_path = init_from
    if kl_weight > 0 and kl_reference_path is None:
        raise ValueError("kl_weight > 0 needs the frozen reference policy's weights: give kl_reference_path or init_from")
    if mwer_lm_path is not None and objective != "mwer":
        raise ValueError("mwer_lm_path belongs to objective='mwer' (the sampled objectives decode without an LM)")
    if kl_weight > 0 and objective == "mwer":
        raise ValueError("objective='mwer' does not take kl_weight (the KL penalty belongs to the sampled objectives)")
    print("Num epochs:", num_epochs, "Batch size:", batch_size)
    alphabet_path = os.path.join(corpus_path, "alphabet.txt") if units_path is None else units_path
    alphabet, char2ind = _read_alphabet(alphabet_path)
    units = None
    if units_path is not None:
        from .units import SubwordUnits
        units = SubwordUnits.load(units_path)
        if units.unit2ind != {k: v for k, v in char2ind.items() if v > 0}:
            raise ValueError(f"{units_path}: not a units file (one distinct, non-empty unit per line)")
    if wide_alphabet is None:
        wide_alphabet = len(char2ind) > hipops.MAX_VOCAB_NARROW
    wide_alphabet = bool(wide_alphabet)
    resume_state = None
    if wide_sequence is None:
        wide_sequence = False
        last = os.path.join(model_path, "checkpoint_last.pth")
        if wide_alphabet and resume and os.path.exists(last):           # a resumed run keeps the objective it was started with:
            resume_state = torch.load(last, map_location="cpu")         # the one load of the checkpoint, used again below
            wide_sequence = bool(resume_state.get("wide_sequence", False))
    wide_sequence = bool(wide_sequence)
    if wide_sequence and not wide_alphabet:
        raise ValueError("wide_sequence=True opens the sequence-level objectives for alphabets of more than 64 symbols: it needs wide_alphabet")
    if wide_alphabet and objective == "mwer" and not wide_sequence:
        raise ValueError("objective='mwer' takes an alphabet of at most 64 symbols (the beam search's limit): not with wide_alphabet")
    if mwer_unit_lm_path is not None and not (objective == "mwer" and wide_sequence):
        raise ValueError("mwer_unit_lm_path belongs to objective='mwer' with wide_sequence=True (the wide search fuses the unit LM)")
    wide_objectives = bool(wide_objectives)
    if wide_objectives and not wide_alphabet:
        raise ValueError("wide_objectives=True opens objectives for alphabets of more than 64 symbols: it needs wide_alphabet")
    step_objectives = bool(step_objectives)
    if reward_mode not in ("utterance", "per_step"):
        raise ValueError("reward_mode must be 'utterance' or 'per_step'")
    word_delimiter = None
    spelling = {}
    if spelled_reward:
        if units is None:
            raise ValueError("spelled_reward=True spells subword units into characters: it needs units_path")
        from .units import UnitSpelling
        spelling = {"unit_spelling": UnitSpelling.load(units_path, os.path.join(corpus_path, "alphabet.txt"))}
        if reward_unit == "word":
            spelling["unit_spelling"].word_delimiter("reward_unit='word'")
    elif reward_unit == "word":
        if " " not in char2ind:
            raise ValueError(f"reward_unit='word' splits words at the alphabet's ' ' symbol, and {alphabet_path} has none")
        word_delimiter = char2ind[" "]
    dev = torch.device("cuda", device if isinstance(device, int) else 0) if not isinstance(device, torch.device) else device
    os.makedirs(model_path, exist_ok=True)
    from .features import SpeedPerturb
    speed_perturb = SpeedPerturb.coerce(speed_perturb)
    n_in = n_feats                                              # the model's input width
    if frame_stack is not None:
        from .features import FrameStack
        frame_stack = FrameStack.coerce(frame_stack)
        n_in = frame_stack.out_feats(n_feats)
    wave_augment = _wave_augment(noise_dir, rir_dir, snr_db, noise_prob, rir_prob, dev)
    unit_args = {} if units is None else {"units": units}       # without a units file: the calls as they were
    # the collate function stacks last, validation batches too
    collate_args = unit_args if frame_stack is None else dict(unit_args, frame_stack=frame_stack)
    collate_custom = functools.partial(_collate, device=dev, features=features, target_rate=target_rate, **collate_args)
    if train_dataset is None:
        train_dataset = Data(os.path.join(corpus_path, "train.tsv"), os.path.join(corpus_path, "clips"), char2ind, **unit_args)
    if dev_dataset is None and os.path.exists(os.path.join(corpus_path, "dev.tsv")):
        dev_dataset = Data(os.path.join(corpus_path, "dev.tsv"), os.path.join(corpus_path, "clips"), char2ind, **unit_args)

    torch.manual_seed(seed)
    model = Seq2Seq(alphabet_size=len(char2ind), n_feats=n_in)
    model.apply(weights)                                            # model.py:202
    model = model.to(dev)
    if frame_stack is None:
        _check_features(features, n_feats, train_dataset)
    else:
        _check_features(features, n_in, train_dataset, stack=frame_stack.stack)
    if objective == "mwer":
        from .mwer import MWERTrainer
        mwer_lm = {}
        if mwer_lm_path is not None:
            from .lm import CharNgramLM
            mwer_lm = {"lm": CharNgramLM.load(mwer_lm_path), "lm_alpha": mwer_lm_alpha, "lm_beta": mwer_lm_beta}
        if wide_sequence:
            mwer_lm["wide_sequence"] = True
            if mwer_unit_lm_path is not None:
                from .lm import UnitNgramLM
                mwer_lm.update(unit_lm=UnitNgramLM.load(mwer_unit_lm_path), lm_alpha=mwer_lm_alpha, lm_beta=mwer_lm_beta)
        trainer = MWERTrainer(model, lr=lr, lam=lam, seed=seed, precision=precision, max_grad_norm=max_grad_norm,
                              beam_size=mwer_beam, nbest=mwer_nbest, risk_unit=reward_unit, word_delimiter=word_delimiter,
                              max_hyp_len=max_hyp_len, num_samples=num_samples, reward_baseline=reward_baseline,
                              score_function=score_function, entropy_weight=entropy_weight,
                              **({"reward_mode": reward_mode} if reward_mode != "utterance" else {}), **mwer_lm, **spelling)
    else:
        kl = {}
        if kl_weight > 0:
            # the frozen reference is a model of its own, loaded from its path -- in a resumed run too
            reference = Seq2Seq(alphabet_size=len(char2ind), n_feats=n_in)
            reference.load_state_dict(torch.load(kl_reference_path, map_location="cpu"))
            kl = {"kl_weight": kl_weight, "kl_reference": reference.to(dev)}
        trainer = PolicyGradientTrainer(model, lr=lr, lam=lam, seed=seed, precision=precision, num_samples=num_samples,
                                        reward_baseline=reward_baseline, reward_unit=reward_unit, word_delimiter=word_delimiter,
                                        max_grad_norm=max_grad_norm, score_function=score_function, max_hyp_len=max_hyp_len,
                                        entropy_weight=entropy_weight, **kl, **({"wide_alphabet": True} if wide_alphabet else {}),
                                        **({"wide_objectives": True} if wide_objectives else {}),
                                        **({"wide_sequence": True} if wide_sequence else {}),
                                        **({"reward_mode": reward_mode} if reward_mode != "utterance" else {}),
                                        **({"step_objectives": True} if step_objectives else {}), **spelling)
    losses, val_losses, best, start_epoch = [], [], 9999999.0, 1
    ckpt = os.path.join(model_path, "checkpoint_last.pth")
    resuming = resume and os.path.exists(ckpt)
    if init_from is not None and not resuming:
        model.load_state_dict(torch.load(init_from, map_location=dev))      # in place: the trainer's flat buffer holds the parameters
        print("Initialised from", init_from)
    if resuming:
        st = resume_state if resume_state is not None else torch.load(ckpt, map_location=dev)
        if frame_stack is not None or st.get("frame_stack") is not None:      # the policy decides the model's width: no warning, a refusal
            if st.get("frame_stack") != (None if frame_stack is None else frame_stack.state()):
                raise ValueError("frame_stack: resuming with frame_stack={} but the checkpoint was written with frame_stack={}".format(
                    None if frame_stack is None else frame_stack.state(), st.get("frame_stack")))
        model.load_state_dict(st["model"])
        from .train_step import FLAG_PAD
        # the checkpoint holds the moments of the PARAMETERS (the flat buffers' leading flag words are not state)
        trainer.exp_avg[FLAG_PAD:].copy_(st["exp_avg"]); trainer.exp_avg_sq[FLAG_PAD:].copy_(st["exp_avg_sq"]); trainer.nstep = st["nstep"]
        trainer.set_applied_steps(st.get("applied_steps", st["nstep"]))     # Adam's bias correction counts applied updates
        # the dropout masks are functions of (seed, call counter): restore both, or a resumed run replays the first
        # epoch's masks and differs from an uninterrupted one
        model.encoder._drop_calls = st.get("drop_calls", 0)
        model.encoder.dropout_seed = st.get("dropout_seed", model.encoder.dropout_seed)
        for k, want in (("lr", lr), ("lam", lam), ("num_samples", num_samples), ("reward_baseline", reward_baseline),
                        ("reward_unit", reward_unit), ("max_grad_norm", max_grad_norm),
                        ("accumulate_steps", accumulate_steps), ("score_function", score_function),
                        ("max_hyp_len", max_hyp_len), ("entropy_weight", entropy_weight), ("kl_weight", kl_weight),
                        ("kl_reference_path", kl_reference_path), ("target_rate", target_rate),
                        ("units_path", units_path), ("wide_alphabet", wide_alphabet), ("wide_objectives", wide_objectives),
                        ("reward_mode", reward_mode), ("step_objectives", step_objectives),
                        ("wide_sequence", wide_sequence), ("spelled_reward", bool(spelled_reward)),
                        ("speed_perturb", None if speed_perturb is None else speed_perturb.state()),
                        ("wave_augment", None if wave_augment is None else wave_augment.state())):
            if k in st and st[k] != want:
                print("Warning: resuming with {}={} but the checkpoint was written with {}".format(k, want, st[k]))
        losses, val_losses, best, start_epoch = st["losses"], st["val_losses"], st["best"], st["epoch"] + 1
        print("Resumed from epoch", st["epoch"])

    print("Start training...")
    for epoch in range(start_epoch, num_epochs + 1):
        model.train()
        lens = dataset_lengths(train_dataset) if bucket_by_length else None
        epoch_dataset, train_collate = train_dataset, collate_custom
        if speed_perturb is not None or wave_augment is not None:      # the draws are addressed by (seed, epoch, index in the corpus)
            from .data import Indexed
            epoch_dataset = Indexed(train_dataset)
            draws = {"speed_perturb": speed_perturb, "seed": seed, "offset": epoch}
            if wave_augment is not None:
                draws["wave_augment"] = wave_augment
            train_collate = functools.partial(_collate, device=dev, features=features, target_rate=target_rate, **draws, **collate_args)
        if lens is not None:      # similar lengths per batch instead of model.py:221's shuffle=True
            sampler = LengthBucketSampler(lens, batch_size, seed=seed)
            sampler.set_epoch(epoch)
            loader = tud.DataLoader(epoch_dataset, batch_sampler=sampler, collate_fn=train_collate)
        else:
            loader = tud.DataLoader(epoch_dataset, batch_size=batch_size, shuffle=True, collate_fn=train_collate)
        acc = torch.zeros((), device=dev)
        unfit = torch.zeros((), dtype=torch.int64, device=dev) if frame_stack is not None else None
        n_steps = -(-len(loader) // accumulate_steps)          # optimizer steps of this epoch
        step, group = 0, []
        for n_batch, batch in enumerate(loader, 1):
            if unfit is not None:      # counted on the device: read once, at the end of the epoch
                unfit += (~frame_stack.fits(batch["trans"], batch["tmask"].sum(1), batch["fmask"].sum((1, 2)))).sum()
            if accumulate_steps == 1:
                loss = trainer.step(*_to_device(batch, dev))
            else:
                group.append(_to_device(batch, dev))
                if len(group) < accumulate_steps and n_batch < len(loader):
                    continue
                loss = trainer.step_accumulated(group)
                group = []
            step += 1
            acc += loss
            if log_every and step % log_every == 0:
                val = float(loss)                      # the host synchronises here anyway: check the sweeps' error words
                hipops.lstm_assert_no_timeouts()       # (until then the guarded Adam has skipped every invalid update)
                line = "Step {}/{}. Loss: {:>4f}".format(step, n_steps, val)
                if max_grad_norm is not None:
                    line += " Grad norm: {:>4f}".format(float(trainer.last_grad_norm))
                if trainer.entropy_weight > 0:
                    line += " Entropy: {:>4f}".format(float(trainer.last_entropy.mean()))
                if kl_weight > 0:
                    line += " KL: {:>4f}".format(float(trainer.last_kl.mean()))
                print(line)
        losses.append(float(acc) / max(step, 1))
        hipops.lstm_assert_no_timeouts()          # .. and before anything of this epoch is written to disk
        streams.release()                         # the host has synchronised: nothing of the last step needs keeping alive
        np.save(os.path.join(model_path, "train_loss.npy"), np.array(losses))
        print("Epoch:{}/{} Training loss:{:>4f}".format(epoch, num_epochs, losses[-1]))
        if unfit is not None:
            print("Epoch:{}/{} Utterances whose transcript does not fit their stacked frames (zero weight): {}".format(
                epoch, num_epochs, int(unfit)))
        if max_grad_norm is not None:
            print("Epoch:{}/{} Clipped steps: {} Skipped (non-finite gradient): {}".format(epoch, num_epochs, *trainer.clip_counts()))

        curr = losses[-1]
        if dev_dataset is not None:                                 # validation (model.py:246-268)
            model.eval()
            vl = torch.zeros((), device=dev)
            vloader = tud.DataLoader(dev_dataset, batch_size=batch_size, shuffle=False, collate_fn=collate_custom)
            with torch.no_grad():
                for batch in vloader:
                    x, t, fmask, tmask = _to_device(batch, dev)
                    logits, in_len = model.logits(x, fmask)
                    l, _, _, _ = pg_ctc_loss(logits, in_len, t.to(torch.int32).contiguous(),
                                             tmask.sum(1).to(torch.int32).contiguous(), lam=0.0)
                    vl += l
            curr = float(vl) / max(len(vloader), 1)
            val_losses.append(curr)
            np.save(os.path.join(model_path, "val_losses.npy"), np.array(val_losses))
            print("Epoch:{}/{} Validation loss:{:>4f}".format(epoch, num_epochs, curr))
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        if curr < best:                                             # model selection (model.py:270-274)
            torch.save(sd, os.path.join(model_path, "model_best.pth"))
            best = curr
        torch.save(sd, os.path.join(model_path, "model_last.pth"))
        from .train_step import FLAG_PAD
        torch.save({"model": sd, "exp_avg": trainer.exp_avg[FLAG_PAD:], "exp_avg_sq": trainer.exp_avg_sq[FLAG_PAD:], "nstep": trainer.nstep,
                    "applied_steps": trainer.applied_steps(),
                    "losses": losses, "val_losses": val_losses, "best": best, "epoch": epoch,
                    "drop_calls": model.encoder._drop_calls, "dropout_seed": model.encoder.dropout_seed,
                    "lr": lr, "lam": lam, "num_samples": num_samples, "reward_baseline": reward_baseline,
                    "reward_unit": reward_unit, "max_grad_norm": max_grad_norm, "accumulate_steps": accumulate_steps,
                    "score_function": score_function, "max_hyp_len": max_hyp_len, "entropy_weight": trainer.entropy_weight,
                    "kl_weight": kl_weight, "kl_reference_path": kl_reference_path, "target_rate": target_rate,
                    "units_path": units_path, "wide_alphabet": wide_alphabet, "wide_objectives": wide_objectives, "wide_sequence": wide_sequence,
                    "reward_mode": reward_mode, "step_objectives": step_objectives,
                    "spelled_reward": bool(spelled_reward),
                    **({} if frame_stack is None else {"frame_stack": frame_stack.state()}),
                    "speed_perturb": None if speed_perturb is None else speed_perturb.state(),
                    "wave_augment": None if wave_augment is None else wave_augment.state()}, ckpt)
    return losses, val_losses


def predict(test_path, aud_path, alphabet_path, model_path, batch_size, maxlen=None, maxlent=None, device_id=0,
            test_dataset=None, n_feats=120, beam_size=5, features="mfcc", lm_path=None, lm_alpha=0.0, lm_beta=0.0,
            nbest=1, rescore_lm_path=None, rescore_alpha=0.0, rescore_beta=0.0, lm_fast=False, target_rate=None,
            mbr=False, mbr_unit="char", mbr_scale=1.0, rescore_word_lm_path=None, rescore_word_alpha=0.0, rescore_word_beta=0.0,
            error_report=False, units_path=None, wide_beam=False, wide_second_pass=False, unit_lm_path=None, unit_lm_alpha=0.0,
            unit_lm_beta=0.0, rescore_unit_lm_path=None, rescore_unit_alpha=0.0, rescore_unit_beta=0.0, spelled=False,
            frame_stack=None, fused_word_lm_path=None, fused_word_alpha=0.0, fused_word_beta=0.0, oov_penalty=0.0,
            word_confidence=False, confidence_pivot="map",
            wide_hotwords=False, hotwords_path=None, hotword_weight=1.0, hotword_boost=1.0):
    """model.py:277-339: load model_best.pth, forward, beam=5 prefix search (device side, batched),
    collapse_fn, CER/WER, predicted.txt.  Frames are cut by the FEATURE mask (the reference cuts the
    time axis by the target mask, model.py:322 -- a listed defect).  Returns (CER, WER).
    features: the front end for items that carry waveforms, as in ``train`` ("mfcc": n_feats=120, "logmel80": n_feats=80);
    the features stay on the device.  target_rate: None (default) or 16000 -- audio at another rate is converted on the device
    first, as in ``train``.
    lm_path: None (default) or an ``lm.npz`` written by ``build_lm`` / ``CharNgramLM.save``: the beam search then adds
    lm_alpha * ln p_lm(s | context) + lm_beta to every extension by a character s (CTCDecoder).
    lm_fast: False (default: with an LM every search takes the workgroup-per-utterance kernel) or True: the single-wave kernel with
    the LM term where its limits allow (beam_size <= 16, at most 64 symbols, T * beam_size <= 24576, T <= 4096; CTCDecoder(fast_lm=)),
    several times faster; scores agree to ~1e-7 relative, hypotheses wherever no two candidates are closer than that.
    nbest: 1 (default: the calls above, nothing else) or N with 2 <= N <= beam_size: the search returns its N best hypotheses per
    utterance (``decode_batch(nbest=N)``), all of them go to ``nbest.tsv`` in model_path -- utterance, rank, first-pass score, second-pass
    total (empty when not rescored), collapsed text, tab-separated -- and the oracle CER (the best hypothesis of every list) is
    printed beside the CER of the chosen one.  rescore_lm_path: None, or an ``lm.npz`` for a second pass over the lists
    (``CTCDecoder.rescore`` with the exact CTC likelihood as acoustic score, total = nll - rescore_alpha * ln p_lm - rescore_beta *
    length): the hypothesis with the lowest total is the one written to predicted.txt and scored.  Without it rank 0 is.
    With nbest > 1 every list comes from the workgroup-per-utterance kernel: rank 0 is ``ctc_beam_search(generic=True)``'s result,
    while nbest = 1 without an LM takes the single-wave fp32 kernel for beam_size <= 16.  The two agree to ~1e-7 relative in their
    scores, so their hypotheses can differ only where two candidates are closer than that.
    mbr: False (default: everything above, nothing else) or True, with nbest >= 2: minimum-Bayes-risk decoding
    (``CTCDecoder.mbr_from_list``).  The posterior over each list is softmax(-mbr_scale * score), score being the rescored total with
    rescore_lm_path and the exact CTC likelihood without; the hypothesis of least expected character (mbr_unit="char") or word
    (mbr_unit="word", words split at the alphabet's " ") edit distance to the rest of its list is the one written to predicted.txt
    and scored, the CER / WER of the best-scored rows are printed beside its own, and ``mbr.tsv`` in model_path gets one line per
    utterance: utterance, chosen rank, its expected errors, rank 0's expected errors, tab-separated.
    rescore_word_lm_path: None (default: everything above, nothing else) or a ``word_lm.npz`` of ``build_word_lm`` /
    ``WordNgramLM.save``, with nbest >= 2: the second pass also scores every hypothesis' words (split at the alphabet's " ") under
    the word n-gram LM, total -= rescore_word_alpha * ln p_word + rescore_word_beta * words (``CTCDecoder.rescore(word_lm=)``), on top
    of the exact CTC likelihood and, with rescore_lm_path, the character LM; with mbr=True the posterior comes from these totals.
    ``nbest.tsv`` then has three more columns: word_logp, n_words, n_oov.
    error_report: False (default: everything above, nothing else) or True: the strings that are scored (reference, collapsed
    hypothesis) are also aligned on the device (``metrics.ErrorReport``), ``errors.txt`` -- per utterance a REF / HYP / OPS triple of
    aligned lines, then the totals -- and ``confusions.tsv`` -- kind, ref, hyp, count, sorted by count -- are written into model_path,
    and one corpus-level line, (S + D + I) / reference length with the S / D / I breakdown for characters and words, is printed after
    the line above.  The return value (the MEAN of the per-utterance rates) and every other output stay what they are.
    beam_size=0: greedy decoding -- arg-max per frame and CTC collapse on the device (``CTCdecoder.greedy_decode``), no search; the only
    decoder for an alphabet of more than 64 symbols (up to 1024) without ``wide_beam``, where beam_size > 0 raises up front.  Not with
    nbest > 1 or an LM.
    units_path: None (default) or a units file (``build_units``) that stands in place of ``alphabet_path``: the references are
    encoded by greedy longest match, the hypotheses are the concatenated units (no ``collapse_fn``: a unit may end with the character the
    next one starts with), and CER / WER are computed on the decoded strings as ever.
    wide_beam: False (default: everything above, nothing else) or True: an alphabet of more than 64 symbols (up to 1024) is searched
    with beam_size > 0 by the exact wide prefix beam search (``CTCDecoder(wide_search=True)``, csrc/beam_wide.hip).  nbest=N then
    writes ``nbest.tsv`` with the first-pass scores, and the oracle error rate over units (the best hypothesis of every list against
    the encoded reference, ``metrics.nbest_oracle``) is printed beside CER / WER.  The wide search has no LM fusion and its lists no
    second pass by default: lm_path, the rescore_* options, mbr and error_report raise for such an alphabet.  Alphabets of at most 64
    symbols are not affected by the flag.
    wide_second_pass: False (default: everything above, nothing else) or True, with wide_beam=True and nbest >= 2: every wide list is
    re-ranked by the exact CTC likelihood of its hypotheses (``CTCDecoder.rescore`` on the forward scorer, csrc/hyp_score.hip), which
    fills the total column of ``nbest.tsv``; the row of lowest total is the one written to predicted.txt and scored.  mbr=True is
    then allowed with mbr_unit="char" -- the risk is counted in units -- and writes ``mbr.tsv``; mbr_unit="word" raises (a unit may
    span a space), and so do lm_path, rescore_lm_path, rescore_word_lm_path and error_report, which stay refused for such an alphabet.
    Alphabets of at most 64 symbols are not affected by the flag.
    unit_lm_path: None (default: everything above, nothing else) or a ``unit_lm.npz`` of ``build_unit_lm`` / ``UnitNgramLM.save``,
    with wide_beam=True and beam_size > 0: the wide search adds unit_lm_alpha * ln p_lm(s | context) + unit_lm_beta to every
    extension by a unit s (``CTCDecoder(wide_search=True, unit_lm=)``, a sparse back-off model over the units themselves); the
    first-pass scores are then fused scores.  An alphabet of at most 64 symbols takes the wide entry with it too.
    rescore_unit_lm_path: None (default: everything above, nothing else) or such a file, with nbest >= 2 (and wide_second_pass=True
    for an alphabet of more than 64 symbols): the second pass also scores every hypothesis under the unit LM, total -=
    rescore_unit_alpha * ln p_unit + rescore_unit_beta * length (``CTCDecoder.rescore(unit_lm=)``); with mbr=True the posterior comes
    from these totals.  ``nbest.tsv`` then has one more column at its end: unit_logp.
    spelled: False (default: everything above, nothing else -- every refusal above stands) or True, with units_path: the lists of a
    subword model are counted on their SPELLED text (``units.UnitSpelling`` from the units file and ``alphabet_path``, the corpus'
    alphabet.txt, where that file exists; else the characters of the units).  error_report=True is then allowed with greedy decoding
    and with the wide search (``ErrorReport`` over the spelling's characters), mbr_unit="word" with wide_second_pass=True (and
    mbr_unit="char" counts characters, not units: ``CTCDecoder.mbr_from_list(unit_spelling=)``), and the oracle of a wide list is
    printed as the CER over spelled text (``metrics.nbest_oracle(spelling=)``).
    hotwords_path: None (default: everything above, nothing else) or a text file with one phrase per line (empty lines are skipped):
    the decoder is biased towards these phrases (``lm.HotwordBias`` with boost = hotword_boost per token, applied with weight
    hotword_weight).  An alphabet of at most 64 symbols: the bias is fused into the beam search (``CTCDecoder(hotwords=)``, beam_size
    >= 1; the first-pass scores are then fused scores) -- not with lm_fast=True or unit_lm_path, whose kernels have no bias.  A wider
    alphabet: with units_path, wide_beam=True and wide_second_pass=True (nbest >= 2) the phrases are encoded with the units, each
    in isolation, and the bias goes into the second pass over the wide lists (``CTCDecoder.rescore(bias=)``); the wide search itself
    takes no bias unless ``wide_hotwords`` is given, so any other combination raises a ValueError that names the missing option.
    wide_hotwords: False (default: everything above, nothing else -- every refusal above stands) or True, with units_path,
    wide_beam=True and hotwords_path (ValueError naming the missing one): the phrases, compiled with the units, are fused into the
    wide search itself (``CTCDecoder(wide_search=True, wide_hotwords=True, hotwords=)``, csrc/beam_wide.hip), together with
    unit_lm_path if given and without needing wide_second_pass; the first-pass scores are then fused scores.  With
    wide_second_pass=True as well the second pass applies ``rescore(bias=)`` as above: the first pass gets the phrase into the list,
    the exact-likelihood second pass ranks it, and ``nbest.tsv`` carries B(y) of every hypothesis as its last column.
    frame_stack: None (default) or (stack, skip[, left]) / a features.FrameStack, as in ``train``.  None takes the policy the model
    was trained with from <model_path>/checkpoint_last.pth, where there is one -- a model trained without a policy, or a directory
    without that file, decodes as ever --; a policy that differs from the checkpoint's raises.  The model then has n_feats * stack
    inputs and every decoder sees ceil(n / skip) frames.
    fused_word_lm_path: None (default: everything above, nothing else) or a word LM's .npz (``lm.WordNgramLM.save``, or a
    ``lm.WordFusion.save`` with its own delimiter and oov_penalty): the model and its vocabulary as a lexicon are fused into the
    first pass itself (``CTCDecoder(fused_word_lm=)``, csrc/beam.hip WORDS = true) -- every word end adds fused_word_alpha * ln p(word |
    history) + fused_word_beta, the way out of the lexicon ``oov_penalty`` (<= 0; -inf: only lexicon words), and the final beam is
    ranked with the pending word and </s> scored; the first-pass scores are then fused scores.  beam_size >= 1, an alphabet of at most
    64 symbols with the ' ' symbol; not together with lm_path, hotwords_path, lm_fast, wide_beam or unit_lm_path (ValueError naming
    the option).  ``rescore_word_lm_path`` stays the second pass it is.
    word_confidence: False (default: everything above, nothing else) or True, with nbest >= 2 and an alphabet of at most 64 symbols
    with the ' ' symbol (ValueError naming what is missing; not for subword models -- units_path --, whose units may hold a space):
    every word of a decoded hypothesis gets its N-best confidence and its time span.  The posterior over each list is
    softmax(-mbr_scale * score) as for ``mbr`` (the rescored totals where there is a second pass, the exact CTC likelihood
    without); the list is aligned to the pivot row -- confidence_pivot="map": the best-scored row, what is written to predicted.txt
    unless mbr=True chooses another; "mbr": the row of least expected character errors -- and a word's confidence is the posterior
    mass of the hypotheses that have the word there (``CTCDecoder.confidence``; csrc/confidence.hip); the pivot rows are force-aligned
    for the spans (``CTCDecoder.align_batch``, ``word_spans``).  ``words.tsv`` in model_path gets one line per word: utterance, word
    index, word, start frame, end frame (one past the last; -1 -1 for an empty word or a row that does not fit its frames),
    confidence -- in INPUT frames under a frame_stack policy, as ``align`` writes them.  The word and character normalised cross
    entropies of the confidences against the transcripts (``metrics.confidence_nce``) are printed.  predicted.txt, the rates and
    every other output stay what they are."""
    import os
    import functools
    import torch.utils.data as tud
    from .CTCdecoder import CTCDecoder, collapse_fn, greedy_decode
    from .lm import CharNgramLM, UnitNgramLM, WordNgramLM
    from .data import Data
    from .data import collate_custom as _collate
    from .metrics import edit_dist_batch, evaluate, save_predictions

    nbest = int(nbest)
    greedy = int(beam_size) == 0
    if greedy:
        if nbest != 1 or lm_path is not None:
            raise ValueError("beam_size=0 decodes greedily: it has no N-best list and no LM (nbest > 1 and lm_path need beam_size >= 1)")
    elif nbest < 1 or nbest > int(beam_size):
        raise ValueError(f"nbest must lie in [1, beam_size = {beam_size}] (got {nbest})")
    if rescore_lm_path is not None and nbest < 2:
        raise ValueError("rescoring needs a list: give nbest >= 2 with rescore_lm_path")
    if rescore_word_lm_path is not None and nbest < 2:
        raise ValueError("rescoring needs a list: give nbest >= 2 with rescore_word_lm_path")
    if rescore_unit_lm_path is not None and nbest < 2:
        raise ValueError("rescoring needs a list: give nbest >= 2 with rescore_unit_lm_path")
    if unit_lm_path is not None and (greedy or not wide_beam):
        raise ValueError("unit_lm_path: the unit LM is fused into the wide beam search; give wide_beam=True and beam_size >= 1")
    if unit_lm_path is not None and lm_path is not None:
        raise ValueError("unit_lm_path: not together with lm_path -- one first-pass language model")
    if mbr and nbest < 2:
        raise ValueError("minimum-Bayes-risk decoding needs a list: give nbest >= 2 with mbr=True")
    if mbr and mbr_unit not in ("char", "word"):
        raise ValueError(f"mbr_unit must be 'char' or 'word' (got {mbr_unit!r})")
    if word_confidence:
        if nbest < 2:
            raise ValueError("word_confidence: the confidences come from an N-best list; give nbest >= 2 with it")
        if units_path is not None:
            raise ValueError("word_confidence: not for subword models (units_path) -- a unit may hold a space, so the list has no "
                             "word boundaries of its own")
        if confidence_pivot not in ("map", "mbr"):
            raise ValueError(f"confidence_pivot must be 'map' or 'mbr' (got {confidence_pivot!r})")
    if wide_hotwords:
        for name, given in (("wide_beam", bool(wide_beam)), ("units_path", units_path is not None),
                            ("hotwords_path", hotwords_path is not None)):
            if not given:
                raise ValueError(f"{name}: wide_hotwords fuses the phrases of hotwords_path into the wide search over units; give "
                                 f"units_path, wide_beam=True and hotwords_path with it")
    if hotwords_path is not None:
        if greedy:
            raise ValueError("hotwords_path: greedy decoding (beam_size=0) has no hotword bias; give beam_size >= 1")
        if lm_fast:
            raise ValueError("lm_fast: the single-wave kernel has no hotword bias; give lm_fast=False with hotwords_path")
        if unit_lm_path is not None and not wide_hotwords:
            raise ValueError("unit_lm_path: the wide search it is fused into has no hotword bias; not together with hotwords_path")
    if fused_word_lm_path is not None:
        if greedy:
            raise ValueError("fused_word_lm_path: greedy decoding (beam_size=0) has no word LM fusion; give beam_size >= 1")
        for name, given in (("lm_path", lm_path is not None), ("hotwords_path", hotwords_path is not None), ("lm_fast", bool(lm_fast)),
                            ("unit_lm_path", unit_lm_path is not None), ("wide_beam", bool(wide_beam)),
                            ("units_path", units_path is not None)):
            if given:
                raise ValueError(f"{name}: not together with fused_word_lm_path -- the word LM is fused into the workgroup kernel's "
                                 f"search over characters, alone")
    char_alphabet_path = alphabet_path
    if units_path is not None:
        alphabet_path = units_path
    alphabet, char2ind = _read_alphabet(alphabet_path)
    if fused_word_lm_path is not None:
        if len(alphabet) > hipops.MAX_VOCAB_NARROW:
            raise ValueError(f"fused_word_lm_path: the fused search takes at most {hipops.MAX_VOCAB_NARROW} symbols and "
                             f"{alphabet_path} has {len(alphabet)}")
        if " " not in char2ind:
            raise ValueError("fused_word_lm_path needs an alphabet with the ' ' symbol")
    ind2char = {char2ind[k]: k for k in char2ind}
    if word_confidence:
        if len(alphabet) > hipops.MAX_VOCAB_NARROW:
            raise ValueError(f"word_confidence: not over {len(alphabet)} > {hipops.MAX_VOCAB_NARROW} symbols -- a subword unit may hold "
                             f"a space")
        if " " not in char2ind:
            raise ValueError("word_confidence needs an alphabet with the ' ' symbol")
    unit_args = {}
    if units_path is not None:
        from .units import SubwordUnits
        unit_args = {"units": SubwordUnits.load(units_path)}
    spelling = None
    if spelled:
        if units_path is None:
            raise ValueError("spelled=True spells subword units into characters: it needs units_path")
        from .units import UnitSpelling
        have = char_alphabet_path is not None and char_alphabet_path != units_path and os.path.isfile(str(char_alphabet_path))
        spelling = UnitSpelling.load(units_path, char_alphabet_path if have else None)
        if (mbr and mbr_unit == "word") or error_report:
            spelling.word_delimiter("mbr_unit='word'" if mbr and mbr_unit == "word" else "error_report")
    wide = len(alphabet) > hipops.MAX_VOCAB_NARROW and not greedy and bool(wide_beam)
    second = wide and bool(wide_second_pass)
    if second:
        if nbest < 2:
            raise ValueError("wide_second_pass re-ranks a list: give nbest >= 2 with it")
        for name, given in (("lm_path", lm_path is not None), ("rescore_lm_path", rescore_lm_path is not None),
                            ("rescore_word_lm_path", rescore_word_lm_path is not None),
                            ("error_report", bool(error_report) and spelling is None)):
            if given:
                raise ValueError(f"{name}: not with the wide beam search ({len(alphabet)} > {hipops.MAX_VOCAB_NARROW} symbols): its "
                                 f"second pass is the exact CTC likelihood and minimum-Bayes-risk decoding over units, without "
                                 f"language models or an error report")
        if mbr and mbr_unit == "word" and spelling is None:
            raise ValueError(f"mbr_unit='word': not over {len(alphabet)} > {hipops.MAX_VOCAB_NARROW} symbols -- a subword unit may span "
                             f"a space; take mbr_unit='char', which counts units")
    elif wide:
        for name, given in (("lm_path", lm_path is not None), ("rescore_lm_path", rescore_lm_path is not None),
                            ("rescore_word_lm_path", rescore_word_lm_path is not None), ("mbr", bool(mbr)),
                            ("error_report", bool(error_report) and spelling is None),
                            ("rescore_unit_lm_path", rescore_unit_lm_path is not None)):
            if given:
                raise ValueError(f"{name}: not with the wide beam search ({len(alphabet)} > {hipops.MAX_VOCAB_NARROW} symbols), which "
                                 f"has no LM fusion, no second pass over its lists and no error report yet")
    hotwords = rescore_bias = None
    if hotwords_path is not None:
        from .lm import HotwordBias
        if len(alphabet) > hipops.MAX_VOCAB_NARROW and not wide_hotwords:
            for name, given in (("units_path", units_path is not None), ("wide_beam", wide), ("wide_second_pass", second)):
                if not given:
                    raise ValueError(f"{name}: hotwords over {len(alphabet)} > {hipops.MAX_VOCAB_NARROW} symbols go into the second pass "
                                     f"over the wide lists (the wide search has no bias); give units_path, wide_beam=True and "
                                     f"wide_second_pass=True with hotwords_path")
        with open(hotwords_path, "r") as fo:
            lines = fo.readlines()
        if units_path is not None:
            bias = HotwordBias.from_units(lines, unit_args["units"], boost=hotword_boost)
        else:
            bias = HotwordBias.from_strings(lines, alphabet, boost=hotword_boost)
        if bias.vocab != len(alphabet):
            raise ValueError(f"hotwords_path: the phrases compile to {bias.vocab} symbols; {alphabet_path} has {len(alphabet)}")
        if len(alphabet) > hipops.MAX_VOCAB_NARROW:      # the second pass over the wide lists, and / or the wide search itself
            rescore_bias = bias if second else None
            hotwords = bias if wide_hotwords else None
        else:
            hotwords = bias
    if len(alphabet) > hipops.MAX_VOCAB_NARROW and not greedy and not wide:
        raise ValueError(f"the beam search takes at most {hipops.MAX_VOCAB_NARROW} symbols and {alphabet_path} has {len(alphabet)}: "
                         f"decode greedily with beam_size=0 (up to {hipops.MAX_VOCAB_WIDE} symbols)")
    dev = torch.device("cuda", device_id)
    frame_stack = _frame_stack_of(model_path, frame_stack, "predict")
    n_in = n_feats if frame_stack is None else frame_stack.out_feats(n_feats)
    model = Seq2Seq(alphabet_size=len(alphabet), n_feats=n_in)
    model.load_state_dict(torch.load(os.path.join(model_path, "model_best.pth"), map_location="cpu"))
    model = model.to(dev).eval()
    if test_dataset is None:
        test_dataset = Data(test_path, aud_path, char2ind, **unit_args)
    if frame_stack is None:
        _check_features(features, n_feats, test_dataset)
    else:
        _check_features(features, n_in, test_dataset, stack=frame_stack.stack)
        if not word_confidence:      # word spans need the input frame counts: the batch is then stacked in the loop, as align does
            unit_args = dict(unit_args, frame_stack=frame_stack)
    collate_custom = functools.partial(_collate, device=dev, features=features, target_rate=target_rate, **unit_args)
    # a units file: the device's collapse is the whole collapse -- collapse_fn would merge a unit's last character with the next unit's first
    to_text = collapse_fn if units_path is None else (lambda text: text)
    loader = tud.DataLoader(test_dataset, batch_size=batch_size, shuffle=False, collate_fn=collate_custom)
    lm = CharNgramLM.load(lm_path) if lm_path is not None else None
    unit_lm = rescore_unit_lm = None
    for name, path in (("unit_lm_path", unit_lm_path), ("rescore_unit_lm_path", rescore_unit_lm_path)):
        if path is not None:
            m = UnitNgramLM.load(path)
            if m.vocab != len(alphabet) or m.blank != 0:
                raise ValueError(f"{name}: the model is over {m.vocab} symbols with blank {m.blank}; {alphabet_path} has "
                                 f"{len(alphabet)} symbols and blank 0")
            if name == "unit_lm_path":
                unit_lm = m
            else:
                rescore_unit_lm = m
    hotword_args = {} if hotwords is None else {"hotwords": hotwords, "hotword_weight": hotword_weight}
    if fused_word_lm_path is not None:
        import numpy as np
        from .lm import WordFusion
        with np.load(fused_word_lm_path, allow_pickle=False) as z:
            is_fusion = "fusion_vocab" in z.files
        fused = WordFusion.load(fused_word_lm_path) if is_fusion else WordNgramLM.load(fused_word_lm_path)
        hotword_args = dict(fused_word_lm=fused, fused_word_alpha=fused_word_alpha, fused_word_beta=fused_word_beta,
                            **({} if is_fusion else {"word_delimiter": char2ind[" "], "oov_penalty": oov_penalty}))
    if unit_lm is not None:
        decoder = CTCDecoder(alphabet, lm_alpha=unit_lm_alpha, lm_beta=unit_lm_beta, wide_search=True, unit_lm=unit_lm,
                             wide_hotwords=bool(wide_hotwords), **hotword_args)
    else:
        decoder = CTCDecoder(alphabet, lm=lm, lm_alpha=lm_alpha, lm_beta=lm_beta, fast_lm=bool(lm_fast), wide_search=wide,
                             wide_hotwords=bool(wide_hotwords) and wide, **hotword_args)
    list_text = to_text if wide else collapse_fn      # a wide list holds units: their concatenation is the text
    if mbr and mbr_unit == "word" and spelling is None and " " not in char2ind:
        raise ValueError("mbr_unit='word' needs an alphabet with the ' ' symbol")
    rescore_lm = CharNgramLM.load(rescore_lm_path) if rescore_lm_path is not None else None
    if rescore_word_lm_path is not None and " " not in char2ind:
        raise ValueError("rescore_word_lm_path needs an alphabet with the ' ' symbol")
    word_lm = WordNgramLM.load(rescore_word_lm_path) if rescore_word_lm_path is not None else None
    word_args = {} if word_lm is None else {"word_lm": word_lm, "word_lm_alpha": rescore_word_alpha, "word_lm_beta": rescore_word_beta,
                                            "word_delimiter": char2ind[" "]}
    if rescore_unit_lm is not None:
        word_args = dict(word_args, unit_lm=rescore_unit_lm, unit_lm_alpha=rescore_unit_alpha, unit_lm_beta=rescore_unit_beta)
    if rescore_bias is not None:
        word_args = dict(word_args, bias=rescore_bias, bias_weight=float(hotword_weight))
    report = None
    if error_report:
        from .metrics import ErrorReport
        report = (ErrorReport([a.replace("\n", "") for a in alphabet], " ", device=dev) if spelling is None else
                  ErrorReport(spelling.char_alphabet, " ", device=dev))
    targets, predicted, tot_cer, tot_wer, n = [], [], 0.0, 0.0, 0
    nbest_lines, tot_oracle = [], 0.0
    mbr_lines, map_cer, map_wer = [], 0.0, 0.0
    word_lines, conf_pairs = [], {"word": ([], []), "char": ([], [])}
    print("Total number of examples: ", len(test_dataset))
    with torch.no_grad():
        for step, batch in enumerate(loader, 1):
            print("Decoding step {}/{}...".format(step, len(loader)))
            x, t, fmask, tmask = _to_device(batch, dev)
            if word_confidence and frame_stack is not None:
                n_frames = fmask.sum(1).to(torch.int64).cpu()
                x, fmask = frame_stack(x.to(torch.float32).contiguous(), fmask)
                fmask = fmask.squeeze(1)
            logits, in_len = model.logits(x, fmask)
            lp = Fh.LogSoftmaxFn.apply(logits)
            if nbest > 1:
                nb = decoder.decode_batch(lp, in_len, beam_size=beam_size, nbest=nbest)
                tok, tl, total, words, units_lp, bias_col = nb.tokens[0], nb.lengths[0], None, None, None, None
                if rescore_lm is not None or word_lm is not None or second or rescore_unit_lm is not None:
                    rs = decoder.rescore(lp, in_len, nb, lm=rescore_lm, lm_alpha=rescore_alpha if rescore_lm is not None else 0.0,
                                         lm_beta=rescore_beta if rescore_lm is not None else 0.0, **word_args)
                    tok, tl, total = rs.best_tokens, rs.best_len, rs.total.cpu()
                    if word_lm is not None:
                        words = (rs.word_logp.cpu(), rs.n_words.cpu(), rs.n_oov.cpu())
                    if rescore_unit_lm is not None:
                        units_lp = rs.unit_logp.cpu()
                    if wide_hotwords and rescore_bias is not None:
                        bias_col = rs.bias.cpu()
                if mbr:
                    score = rs.total if total is not None else decoder.rescore(lp, in_len, nb, lm=None).total
                    if spelling is not None:
                        md = decoder.mbr_from_list(nb, score, vocab=lp.shape[2], risk_unit=mbr_unit, posterior_scale=mbr_scale,
                                                   unit_spelling=spelling)
                    else:
                        md = decoder.mbr_from_list(nb, score, vocab=lp.shape[2], risk_unit=mbr_unit, posterior_scale=mbr_scale,
                                                   word_delimiter=char2ind[" "] if mbr_unit == "word" else None)
                    map_tok, map_tl, tok, tl = tok.cpu(), tl.cpu(), md.tokens, md.lengths
                    mbest, mrisk = md.best.cpu(), md.risk.cpu()
                    for i in range(mbest.shape[0]):
                        mbr_lines.append("{}\t{}\t{:.6f}\t{:.6f}\n".format(n + i, int(mbest[i]), float(mrisk[int(mbest[i]), i]),
                                                                          float(mrisk[0, i])))
                if word_confidence:
                    from .metrics import hyp_correct
                    if mbr and mbr_unit == "char":
                        cmd = md
                    else:
                        score = rs.total if total is not None else decoder.rescore(lp, in_len, nb, lm=None).total
                        cmd = decoder.mbr_from_list(nb, score, vocab=lp.shape[2], risk_unit="char", posterior_scale=mbr_scale)
                    if confidence_pivot == "mbr":
                        piv = cmd.best
                    else:      # the best-scored row: the second pass' first where there is one, the search's otherwise
                        piv = rs.order[:, 0].to(torch.int32) if total is not None else torch.zeros_like(cmd.best)
                    wlists, cc, wc = decoder.words_of_list(cmd, lp.contiguous(), in_len, pivot=piv, word_delimiter=char2ind[" "])
                    t32, tl32 = t.to(torch.int32).contiguous(), tmask.sum(1).to(torch.int32).contiguous()
                    for kind, c, delim in (("char", cc, None), ("word", wc, char2ind[" "])):
                        right, n_pos = hyp_correct(t32, tl32, cc.tokens, cc.lengths, unit=kind, delimiter=delim)
                        keep = torch.arange(right.shape[1], device=dev).view(1, -1) < n_pos.view(-1, 1)
                        conf_pairs[kind][0].append(c.conf[:, :right.shape[1]][keep].cpu())
                        conf_pairs[kind][1].append(right[keep].cpu())
                    for i, wl in enumerate(wlists):
                        for j, (word, s0, s1, wconf, _) in enumerate(wl):
                            if frame_stack is not None and s0 >= 0:
                                s0, s1 = frame_stack.input_span(s0, s1, n_frames[i])
                            word_lines.append("{}\t{}\t{}\t{}\t{}\t{:.6f}\n".format(n + i, j, word, s0, s1, wconf))
                # every hypothesis through collapse_fn on the host (the list is copied once); the oracle is over these strings,
                # one edit-distance launch per batch
                ntok, nlen, nscore, ncount = nb.tokens.cpu(), nb.lengths.cpu(), nb.score.cpu(), nb.count.cpu()
                t_h, tlen_h = t.cpu(), tmask.sum(1).cpu()
                refs, hyps, owner = [], [], []
                for i in range(ntok.shape[1]):
                    target = "".join(ind2char[int(k)] for k in t_h[i][:int(tlen_h[i])])
                    for r in range(int(ncount[i])):
                        text = list_text("".join(ind2char[int(k)] for k in ntok[r, i, :nlen[r, i]]))
                        refs.append(target); hyps.append(text); owner.append(i)
                        extra = "" if words is None else "\t{:.6f}\t{}\t{}".format(float(words[0][r, i]), int(words[1][r, i]),
                                                                                  int(words[2][r, i]))
                        if units_lp is not None:
                            extra += "\t{:.6f}".format(float(units_lp[r, i]))
                        if bias_col is not None:
                            extra += "\t{:.6f}".format(float(bias_col[r, i]))
                        nbest_lines.append("{}\t{}\t{:.6f}\t{}\t{}{}\n".format(n + i, r, float(nscore[r, i]),
                                                                            "" if total is None else "{:.6f}".format(float(total[r, i])),
                                                                            text, extra))
                if wide:      # over units: the lists against the encoded references, on the device
                    from .metrics import nbest_oracle
                    if spelling is not None:      # .. or, spelled, over the characters of the text
                        od, _, oc = nbest_oracle(t.to(torch.int32).contiguous(), tmask.sum(1).to(torch.int32).contiguous(), nb,
                                                 spelling=spelling)
                        tot_oracle += sum(int(d) / max(int(c), 1) for d, c in zip(od.cpu().tolist(), oc.cpu().tolist()))
                    else:
                        od, _ = nbest_oracle(t.to(torch.int32).contiguous(), tmask.sum(1).to(torch.int32).contiguous(), nb)
                        tot_oracle += sum(int(d) / max(int(tlen_h[i]), 1) for i, d in enumerate(od.cpu().tolist()))
                else:
                    best = {}
                    for i, d in zip(owner, edit_dist_batch(refs, hyps, device=dev)):
                        best[i] = min(d, best.get(i, d))
                    tot_oracle += sum(d / max(int(tlen_h[i]), 1) for i, d in best.items())
            elif greedy:
                tok, tl = greedy_decode(lp, in_len)
            else:
                tok, tl, _ = decoder.decode_batch(lp, in_len, beam_size=beam_size)
            tok, tl, t, tmask = tok.cpu(), tl.cpu(), t.cpu(), tmask.cpu()
            for i in range(tok.shape[0]):
                seq = to_text("".join(ind2char[int(k)] for k in tok[i, :tl[i]]))
                target = "".join(ind2char[int(k)] for k in t[i][:int(tmask[i].sum())])
                targets.append(target); predicted.append(seq)
                cer, wer = evaluate(target, seq)
                tot_cer += cer; tot_wer += wer; n += 1
                if mbr:
                    cer, wer = evaluate(target, list_text("".join(ind2char[int(k)] for k in map_tok[i, :map_tl[i]])))
                    map_cer += cer; map_wer += wer
            if report is not None:
                report.add(targets[-tok.shape[0]:], predicted[-tok.shape[0]:])
    save_predictions(targets, predicted, model_path)
    cer, wer = tot_cer / max(n, 1), tot_wer / max(n, 1)
    if nbest > 1:
        with open(os.path.join(model_path, "nbest.tsv"), "w") as fo:
            fo.writelines(nbest_lines)
        if mbr:
            with open(os.path.join(model_path, "mbr.tsv"), "w") as fo:
                fo.writelines(mbr_lines)
            print("MBR ({}) CER: {:>4f} WER: {:>4f} MAP CER: {:>4f} WER: {:>4f} Oracle {} ({}-best): {:>4f}".format(
                "unit" if wide and spelling is None else mbr_unit, cer, wer, map_cer / max(n, 1), map_wer / max(n, 1),
                "unit error rate" if wide and spelling is None else "CER", nbest, tot_oracle / max(n, 1)))
        elif wide and spelling is None:
            print("CER: {:>4f} WER: {:>4f} Oracle unit error rate ({}-best): {:>4f}".format(cer, wer, nbest, tot_oracle / max(n, 1)))
        else:
            print("CER: {:>4f} WER: {:>4f} Oracle CER ({}-best): {:>4f}".format(cer, wer, nbest, tot_oracle / max(n, 1)))
    else:
        print("CER: {:>4f} WER: {:>4f}".format(cer, wer))
    if report is not None:
        report.write(model_path)
        print("Corpus " + "  ".join(report.totals_lines()))
    if word_confidence:
        from .metrics import confidence_nce
        with open(os.path.join(model_path, "words.tsv"), "w") as fo:
            fo.writelines(word_lines)
        nce = {k: confidence_nce(torch.cat(v[0]), torch.cat(v[1])) if v[0] else float("nan") for k, v in conf_pairs.items()}
        print("Confidence ({}-best, pivot {}) word NCE: {:>4f} character NCE: {:>4f}".format(nbest, confidence_pivot, nce["word"],
                                                                                           nce["char"]))
    return cer, wer


def align(test_path, aud_path, alphabet_path, model_path, batch_size, maxlen=None, maxlent=None, device_id=0,
          test_dataset=None, n_feats=120, features="mfcc", out_path=None, target_rate=None, frame_stack=None):
    """Forced alignment of the REFERENCE transcripts: ``predict``'s loading and batching, then per batch forward, log-softmax and
    ``CTCDecoder.align_batch`` (Viterbi on the device).  Writes ``out_path`` (default <model_path>/alignments.tsv), one line per
    reference character: utterance index, character index, symbol, start frame, end frame (one past the last), mean log-prob of
    its frames.  An utterance whose transcript does not fit its frames is written with spans -1 -1 and mean -inf, not dropped.
    Returns the per-utterance scores (negative log-probability of the best alignment, +inf where there is none).
    target_rate: as in ``predict``.
    frame_stack: as in ``predict`` (None: the policy in <model_path>/checkpoint_last.pth, where there is one).  The alignment then
    runs over the stacked frames, and a token's span [s', e') is written in INPUT frames, ``FrameStack.input_span``: start s' * skip,
    end min(e' * skip, n) -- stacked frame t' is anchored at input frame t' * skip (its stack covers t'*skip - left .. t'*skip - left
    + stack - 1) --, so the columns of ``alignments.tsv`` keep their meaning of 10 ms frames and consecutive tokens still tile."""
    import os
    import functools
    import torch.utils.data as tud
    from .CTCdecoder import CTCDecoder
    from .data import Data
    from .data import collate_custom as _collate

    alphabet, char2ind = _read_alphabet(alphabet_path)
    ind2char = {char2ind[k]: k for k in char2ind}
    dev = torch.device("cuda", device_id)
    frame_stack = _frame_stack_of(model_path, frame_stack, "align")
    n_in = n_feats if frame_stack is None else frame_stack.out_feats(n_feats)
    model = Seq2Seq(alphabet_size=len(alphabet), n_feats=n_in)
    model.load_state_dict(torch.load(os.path.join(model_path, "model_best.pth"), map_location="cpu"))
    model = model.to(dev).eval()
    if test_dataset is None:
        test_dataset = Data(test_path, aud_path, char2ind)
    if frame_stack is None:
        _check_features(features, n_feats, test_dataset)
    else:
        _check_features(features, n_in, test_dataset, stack=frame_stack.stack)
    collate_custom = functools.partial(_collate, device=dev, features=features, target_rate=target_rate)
    loader = tud.DataLoader(test_dataset, batch_size=batch_size, shuffle=False, collate_fn=collate_custom)
    decoder = CTCDecoder(alphabet)
    scores, lines = [], []
    with torch.no_grad():
        for batch in loader:
            x, t, fmask, tmask = _to_device(batch, dev)
            if frame_stack is not None:      # stacked here, not in the collate function: the spans need the input frame counts
                n_frames = fmask.sum(1).to(torch.int64).cpu()
                x, fmask = frame_stack(x.to(torch.float32).contiguous(), fmask)
                fmask = fmask.squeeze(1)
            logits, in_len = model.logits(x, fmask)
            lp = Fh.LogSoftmaxFn.apply(logits).contiguous()
            tl = tmask.sum(1).to(torch.int32).contiguous()
            a = decoder.align_batch(lp, t.to(torch.int32).contiguous(), tl, in_len)
            t, tl = t.cpu(), tl.cpu()
            st, en, sm, sc = a.token_start.cpu(), a.token_end.cpu(), a.token_logp.cpu(), a.score.cpu()
            for i in range(t.shape[0]):
                u = len(scores)
                scores.append(float(sc[i]))
                for j in range(int(tl[i])):
                    s0, s1 = int(st[i, j]), int(en[i, j])
                    mean = float(sm[i, j]) / (s1 - s0) if s0 >= 0 else -float("inf")
                    if frame_stack is not None and s0 >= 0:
                        s0, s1 = frame_stack.input_span(s0, s1, n_frames[i])
                    lines.append("{}\t{}\t{}\t{}\t{}\t{:.6f}\n".format(u, j, ind2char[int(t[i, j])], s0, s1, mean))
    if out_path is None:
        out_path = os.path.join(model_path, "alignments.tsv")
    with open(out_path, "w") as fo:
        fo.writelines(lines)
    return scores


def build_units(corpus_path, n_units, out_path=None, train_dataset=None):
    """Learn ``n_units`` subword units by byte-pair encoding (``units.SubwordUnits.learn_bpe``) from the training transcripts -- the
    "sentence" column of <corpus_path>/train.tsv, or the "trans" of ``train_dataset``'s items -- starting from the characters of
    <corpus_path>/alphabet.txt, and write them to ``out_path`` (default <corpus_path>/units.txt) for ``train(units_path=)`` and
    ``predict(units_path=)``.  The output layer then has n_units + 1 symbols (at most 1024).  Returns the ``SubwordUnits``."""
    import os
    from .units import SubwordUnits
    _, char2ind = _read_alphabet(os.path.join(corpus_path, "alphabet.txt"))
    base = [c for c, i in sorted(char2ind.items(), key=lambda kv: kv[1]) if i > 0]
    if int(n_units) + 1 > hipops.MAX_VOCAB_WIDE:
        raise ValueError(f"n_units = {n_units}: the output layer takes at most {hipops.MAX_VOCAB_WIDE} symbols, the blank included")
    if train_dataset is not None:
        lines = [train_dataset[i]["trans"] for i in range(len(train_dataset))]
    else:
        import pandas as pd
        lines = [str(x) for x in pd.read_csv(os.path.join(corpus_path, "train.tsv"), sep="\t")["sentence"]]
    units = SubwordUnits.learn_bpe(lines, n_units, alphabet=base)
    units.save(out_path or os.path.join(corpus_path, "units.txt"))
    return units


def build_lm(corpus_path, order=3, out_path=None, train_dataset=None):
    """Character n-gram LM (lm.CharNgramLM, interpolated Witten-Bell) from the transcripts that Data(train.tsv) yields, over the
    symbols of <corpus_path>/alphabet.txt (``<pad>`` = blank = 0); saved to ``out_path`` (default <corpus_path>/lm.npz) for
    ``predict(lm_path=...)``.  ``train_dataset``: any Dataset whose items carry "trans", instead of train.tsv.  Returns the LM."""
    import os
    from .data import Data
    from .lm import CharNgramLM
    _, char2ind = _read_alphabet(os.path.join(corpus_path, "alphabet.txt"))
    if train_dataset is None:
        train_dataset = Data(os.path.join(corpus_path, "train.tsv"), os.path.join(corpus_path, "clips"), char2ind)
    lines = [train_dataset[i]["trans"] for i in range(len(train_dataset))]
    lm = CharNgramLM.from_text(lines, char2ind, order=order, blank=0)
    lm.save(out_path if out_path is not None else os.path.join(corpus_path, "lm.npz"))
    return lm


def build_word_lm(corpus_path, order=3, min_count=1, out_path=None, train_dataset=None):
    """Word n-gram LM (lm.WordNgramLM, interpolated Witten-Bell in back-off form) from the transcripts that Data(train.tsv) yields,
    words split at " " and spelled in the symbols of <corpus_path>/alphabet.txt; saved to ``out_path`` (default
    <corpus_path>/word_lm.npz, beside ``build_lm``'s lm.npz) for ``predict(rescore_word_lm_path=...)``.  Words seen fewer than
    ``min_count`` times count as <unk>.  ``train_dataset``: any Dataset whose items carry "trans", instead of train.tsv.
    Returns the LM."""
    import os
    from .data import Data
    from .lm import WordNgramLM
    _, char2ind = _read_alphabet(os.path.join(corpus_path, "alphabet.txt"))
    if train_dataset is None:
        train_dataset = Data(os.path.join(corpus_path, "train.tsv"), os.path.join(corpus_path, "clips"), char2ind)
    lines = [train_dataset[i]["trans"] for i in range(len(train_dataset))]
    lm = WordNgramLM.from_text(lines, char2ind, order=order, min_count=min_count, delimiter=" ", blank=0)
    lm.save(out_path if out_path is not None else os.path.join(corpus_path, "word_lm.npz"))
    return lm


def build_unit_lm(corpus_path, units_path, order=3, min_count=1, out_path=None, train_dataset=None):
    """Back-off n-gram LM over subword units (lm.UnitNgramLM, interpolated Witten-Bell in back-off form) from the training
    transcripts -- the "sentence" column of <corpus_path>/train.tsv, or the "trans" of ``train_dataset``'s items -- encoded by the
    units of ``units_path`` (``build_units``; blank = 0); saved to ``out_path`` (default <corpus_path>/unit_lm.npz) for
    ``predict(unit_lm_path=...)`` and ``predict(rescore_unit_lm_path=...)``.  An n-gram of order >= 2 seen fewer than ``min_count``
    times is not stored.  Returns the LM."""
    import os
    from .lm import UnitNgramLM
    from .units import SubwordUnits
    units = SubwordUnits.load(units_path)
    if train_dataset is not None:
        lines = [train_dataset[i]["trans"] for i in range(len(train_dataset))]
    else:
        import pandas as pd
        lines = [str(x) for x in pd.read_csv(os.path.join(corpus_path, "train.tsv"), sep="\t")["sentence"]]
    lm = UnitNgramLM.from_text(lines, units, order=order, blank=0, min_count=min_count)
    lm.save(out_path if out_path is not None else os.path.join(corpus_path, "unit_lm.npz"))
    return lm
