"""Low-frame-rate input in numpy: the statement of include/pgasr_hip.h, A0-LFR (pgasr_frame_stack, features.FrameStack), vectorised
over features, offsets and frames.  A plain module: no test, no fixture.  Also the policy and the corpus size of the train-driver
test, which the CPU suite proves to lose no utterance (tests/test_frame_stack_cpu.py)."""
import numpy as np

# (stack, skip, left) of the driver test on pg_harness.tiny_corpus: SyntheticSpeech gives every character 4 .. 8 frames, so n >= 4 L
# and n' = ceil(n / 2) >= 2 L > L + repeats (repeats <= L - 1): every transcript still fits at skip = 2
DRIVER_POLICY = (3, 2, 1)
DRIVER_UTTERANCES = 32


def out_frames(n, skip):
    return -(-int(n) // int(skip))


def frame_stack_ref(x, n_frames, stack, skip, left=0):
    """x (B,F,T), n_frames (B) -> (out (B, stack*F, Tout) of x's dtype, fmask_out (B,1,Tout) float32, n_out (B) int32):
    out[b, j*F + f, t'] = x[b, f, clip(t'*skip + j - left, 0, n-1)] for t' < n' = ceil(n / skip), exactly 0 beyond; n clipped to [0,T]."""
    x = np.asarray(x)
    B, F, T = x.shape
    Tout = out_frames(T, skip)
    out = np.zeros((B, stack * F, Tout), dtype=x.dtype)
    fmask = np.zeros((B, 1, Tout), dtype=np.float32)
    n_out = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = int(np.clip(n_frames[b], 0, T))
        m = n_out[b] = out_frames(n, skip)
        if m == 0:
            continue
        idx = np.clip(np.arange(m)[None, :] * skip + np.arange(stack)[:, None] - left, 0, n - 1)      # (stack, n')
        out[b, :, :m] = x[b][:, idx].transpose(1, 0, 2).reshape(stack * F, m)                          # x[b][:, idx]: (F, stack, n')
        fmask[b, 0, :m] = 1.0
    return out, fmask, n_out


def frame_stack_loops(x, n_frames, stack, skip, left=0):
    """The same statement as three plain loops (small cases only)."""
    x = np.asarray(x)
    B, F, T = x.shape
    Tout = out_frames(T, skip)
    out = np.zeros((B, stack * F, Tout), dtype=x.dtype)
    for b in range(B):
        n = min(max(int(n_frames[b]), 0), T)
        for t in range(out_frames(n, skip)):
            for j in range(stack):
                for f in range(F):
                    out[b, j * F + f, t] = x[b, f, min(max(t * skip + j - left, 0), n - 1)]
    return out


def same_bits(a, b):
    """Equal shape, dtype and bit patterns (NaN payloads and the sign of zero included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def ctc_feasible(labels, n, blank=0):
    """Brute force: is there a CTC alignment of ``labels`` over n frames?  The reachable-state recursion over the blank-extended
    sequence (start in the first two states, stay, advance by one, skip a blank between different symbols), frame by frame."""
    ext = [blank]
    for s in labels:
        ext += [int(s), blank]
    S = len(ext)
    if n <= 0:
        return False
    reach = [i < 2 for i in range(S)]
    for _ in range(n - 1):
        nxt = [False] * S
        for i in range(S):
            if reach[i]:
                nxt[i] = True
                if i + 1 < S:
                    nxt[i + 1] = True
                if i + 2 < S and ext[i + 2] != blank and ext[i + 2] != ext[i]:
                    nxt[i + 2] = True
        reach = nxt
    return reach[S - 1] or (S > 1 and reach[S - 2])
