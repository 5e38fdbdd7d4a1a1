"""The status grid of the CTC loss section: which status each gradient, loss and hypothesis-lattice entry returns for which arguments,
and what the three workspace-size queries return, without a GPU.

Every call has its arrays in HOST memory.  A call that passes every check has no workspace, or one a byte short (for the entries with
two workspaces also: the target's full, the hypotheses' short or missing), and stops at PGASR_ERR_WORKSPACE: no call reaches HIP.
``cases(entry)`` lists (label, overrides of ``base(entry)``) and ``status(lib, entry, overrides)`` makes the call;
tests/test_ctc_status_cpu.py replays the grid against tests/golden/ctc_status_grid.json, which tools/dev/ctc_status_record.py writes
from another commit's library.
"""
import numpy as np

# entry -> (kind, vmax, tail pointers in the signature).  Kinds: "one" (a single optional path), "multi", "seq", "nbest" are the
# gradient passes; "loss" the lattice with an optional gradient; "hyp" the hypothesis lattices.
ENTRIES = {
    "pgasr_ctc_grad_from_lattice": ("one", 64, 0),
    "pgasr_ctc_grad_from_lattice_ent": ("one", 64, 1),
    "pgasr_ctc_grad_from_lattice_kl": ("one", 64, 3),
    "pgasr_ctc_grad_from_lattice_wide": ("one", 1024, 0),
    "pgasr_ctc_grad_from_lattice_multi": ("multi", 64, 0),
    "pgasr_ctc_grad_from_lattice_multi_ent": ("multi", 64, 1),
    "pgasr_ctc_grad_from_lattice_multi_kl": ("multi", 64, 3),
    "pgasr_ctc_grad_from_lattice_multi_wide": ("multi", 1024, 3),
    "pgasr_ctc_grad_from_lattice_multi_steps": ("multi", 1024, 3),
    "pgasr_ctc_grad_from_lattices_seq": ("seq", 64, 0),
    "pgasr_ctc_grad_from_lattices_seq_ent": ("seq", 64, 1),
    "pgasr_ctc_grad_from_lattices_seq_kl": ("seq", 64, 3),
    "pgasr_ctc_grad_from_lattices_seq_wide": ("seq", 1024, 3),
    "pgasr_ctc_grad_from_lattices_nbest": ("nbest", 64, 0),
    "pgasr_ctc_loss_grad": ("loss", 64, 0),
    "pgasr_ctc_loss_grad_wide": ("loss", 1024, 0),
    "pgasr_ctc_hyp_lattice": ("hyp", 64, 0),
    "pgasr_ctc_hyp_lattice_wide": ("hyp", 1024, 0),
}
GRADIENTS = [e for e, k in ENTRIES.items() if k[0] in ("one", "multi", "seq", "nbest")]
SIZES = ["pgasr_ctc_workspace_bytes", "pgasr_ctc_hyp_workspace_bytes", "pgasr_ctc_hyp_workspace_bytes_wide"]
OVERFLOW = dict(K=16, B=33554432)                 # K*B just over 0x7fffffff / 4

_DUMMY = np.zeros(1 << 16, dtype=np.uint8)        # what every non-NULL array argument points to: nothing is read before a refusal
_TAILS = ("ent", "ref", "kl")


def base(entry):
    """Arguments that pass every check of the entry (True / False: an array or NULL); ws, hws: None, "short" or "full"."""
    kind, vmax, _ = ENTRIES[entry]
    paths = kind in ("multi", "seq")
    return dict(lp=True, targets=True, il=True, tl=True, T=6, B=3, V=5 if vmax == 64 else 70, Lmax=4, blank=0, utt=True,
                K=2, pg_coef=kind != "one" and kind != "loss", pg_paths=paths, per_frame=0, hyp_tokens=True, hyp_len=True, Lh=3,
                hyp_stride=None, ent=False, ref=False, kl=False, nll=True, grad=True, ws=None, hws=None)      # hyp_stride None: max(Lh, 1)


def _fields(entry):
    """The arguments the entry's signature has, by their names in ``base``."""
    kind, _, ntail = ENTRIES[entry]
    f = {"lp", "il", "T", "B", "V", "blank"}
    if kind == "hyp":
        return f | {"hyp_tokens", "hyp_stride", "hyp_len", "K", "Lh", "nll", "hws"}
    f |= {"tl", "Lmax", "utt", "pg_coef", "grad", "ws"} | set(_TAILS[:ntail])
    f |= {"loss": {"targets", "pg_paths", "nll"}, "one": {"pg_paths", "per_frame"}, "multi": {"K", "pg_paths"},
          "seq": {"K", "pg_paths", "hyp_len", "Lh", "hws"}, "nbest": {"K", "hyp_len", "Lh", "hws"}}[kind]
    return f


def _all_full(entry, ov):
    """Every workspace the entry takes is full: the one kind of call that could pass every check, which the grid never makes."""
    want = {"hyp": ("hws",), "seq": ("ws", "hws"), "nbest": ("ws", "hws")}.get(ENTRIES[entry][0], ("ws",))
    return all(ov.get(w) == "full" for w in want)


def cases(entry):
    kind, vmax, ntail = ENTRIES[entry]
    has = _fields(entry)
    b = base(entry)
    V = b["V"]
    one = [{}]
    one += [{p: False} for p in ("lp", "targets", "il", "tl", "utt", "grad", "nll", "hyp_tokens", "hyp_len")]
    one += [{"pg_coef": not b["pg_coef"]}, {"pg_paths": not b["pg_paths"]}, {"pg_coef": not b["pg_coef"], "pg_paths": not b["pg_paths"]}]
    one += [{"per_frame": 1}, {"per_frame": 2}, {"per_frame": 1, "pg_coef": True, "pg_paths": True}]
    one += [{"ent": True}, {"ref": True}, {"kl": True}, {"ref": True, "kl": True}, {"ent": True, "ref": True, "kl": True}, {"ent": True, "kl": True}]
    if entry == "pgasr_ctc_grad_from_lattices_seq_wide":          # pg_paths NULL: its N-best form, which has no tails
        one += [dict(t, pg_paths=False) for t in ({"ent": True}, {"ref": True}, {"ref": True, "kl": True}, {"ent": True, "ref": True, "kl": True})]
        one += [{"pg_paths": False, "ws": "full", "hws": "short"}, {"pg_paths": False, "V": vmax + 1}, {"pg_paths": False, "K": 17}]
    one += [{k: v} for k in ("T", "B", "V") for v in (0, -1)]
    one += [{"Lmax": v} for v in (-1, 0, 1023, 1024)] + [{"Lh": v} for v in (-1, 0, 1023, 1024)]
    one += [{"blank": -1}, {"blank": V - 1}, {"blank": V}]
    one += [{"V": v} for v in sorted({64, 65, vmax, vmax + 1})]
    one += [{"K": v} for v in (0, 1, 16, 17)] + [OVERFLOW]
    one += [{"hyp_stride": v} for v in (0, b["Lh"] - 1, b["Lh"], -1)] + [{"hyp_stride": 0, "Lh": 0}]
    one += [{"ws": "short"}, {"hws": "short"}, {"ws": "full", "hws": "short"}, {"ws": "full"}, {"ws": "short", "hws": "full"}]
    # two refusals at once: the order of the checks
    one += [{"lp": False, "V": vmax + 1}, {"K": 0, "V": vmax + 1}, {"Lh": 1024, "Lmax": 1024}, {"blank": -1, "V": vmax + 1},
            {"Lmax": -1, "K": 17}, {"Lmax": -1, "Lh": 1024}, {"blank": V, "Lh": 1024}, {"K": 17, "Lh": 1024}, {"kl": True, "V": vmax + 1},
            {"hyp_len": False, "V": vmax + 1}, {"Lmax": 1024, "ws": "short"}, dict(OVERFLOW, Lmax=1024), dict(OVERFLOW, V=vmax + 1),
            dict(OVERFLOW, T=0), {"hyp_stride": 0, "V": vmax + 1}]
    res = {}
    for ov in one:
        if not set(ov) <= has:
            continue
        if _all_full(entry, ov):
            continue
        res.setdefault(",".join(f"{k}={ov[k]!r}" for k in sorted(ov)) or "base", ov)      # the same call reached twice is one case
    return list(res.items())


def size_cases():
    """The shapes of ``cases`` as arguments of the size queries: (T, B, V, Lmax) and (T, B, V, K, Lh)."""
    b = dict(T=6, B=3, V=5, Lmax=4, K=2, Lh=3)
    one = [{}] + [{k: v} for k in ("T", "B", "V") for v in (0, -1)] + [{k: v} for k in ("Lmax", "Lh") for v in (-1, 0, 1023, 1024)]
    one += [{"V": v} for v in (64, 65, 1024, 1025)] + [{"K": v} for v in (0, 1, 16, 17)] + [OVERFLOW, dict(OVERFLOW, V=1025), {"K": 0, "V": 1025}]
    out = {}
    for name in SIZES:
        keys = ("T", "B", "V", "Lmax") if name == "pgasr_ctc_workspace_bytes" else ("T", "B", "V", "K", "Lh")
        rows = {}
        for ov in one:
            if set(ov) <= set(keys):
                rows.setdefault(",".join(f"{k}={ov[k]!r}" for k in sorted(ov)) or "base", [dict(b, **ov)[k] for k in keys])
        out[name] = list(rows.items())
    return out


def _workspace(lib, need, state):
    """(keep-alive, pointer, bytes) of a host workspace in ``state``."""
    if state is None:
        return None, None, 0
    assert 0 < need < 1 << 28
    keep = np.zeros(need, dtype=np.uint8)
    return keep, keep.ctypes.data, need - (state == "short")


def status(lib, entry, overrides):
    """The entry's status for base(entry) with ``overrides``."""
    kind, vmax, ntail = ENTRIES[entry]
    a = dict(base(entry), **overrides)
    assert not _all_full(entry, a)
    ptr = lambda on: _DUMMY.ctypes.data if on else None      # noqa: E731
    T, B, V, K, Lh =a["T"], a["B"], a["V"], a["K"], a["Lh"]
    hyp_need = getattr(lib, "pgasr_ctc_hyp_workspace_bytes" + ("_wide" if vmax > 64 else ""))
    keep_h, hws, hws_bytes = _workspace(lib, hyp_need(T, B, V, K, Lh) if a["hws"] else 0, a["hws"])
    if kind == "hyp":
        stride = max(Lh, 1) if a["hyp_stride"] is None else a["hyp_stride"]
        st = getattr(lib, entry)(ptr(a["lp"]), ptr(a["hyp_tokens"]), stride, ptr(a["hyp_len"]), ptr(a["il"]), T, B, V, K, Lh, a["blank"],
                                 ptr(a["nll"]), hws, hws_bytes, None)
        del keep_h
        return st
    keep, ws, ws_bytes = _workspace(lib, lib.pgasr_ctc_workspace_bytes(T, B, V, a["Lmax"]) if a["ws"] else 0, a["ws"])
    head = [ptr(a["lp"])] + ([ptr(a["targets"])] if kind == "loss" else []) + [ptr(a["il"]), ptr(a["tl"]), T, B, V, a["Lmax"], a["blank"],
                                                                             ptr(a["utt"])]
    mid = {"loss": [ptr(a["pg_coef"]), ptr(a["pg_paths"]), ptr(a["nll"])],
           "one": [ptr(a["pg_coef"]), ptr(a["pg_paths"]), a["per_frame"]],
           "multi": [K, ptr(a["pg_coef"]), ptr(a["pg_paths"])],
           "seq": [K, ptr(a["pg_coef"]), ptr(a["pg_paths"]), ptr(a["hyp_len"]), Lh],
           "nbest": [K, ptr(a["pg_coef"]), ptr(a["hyp_len"]), Lh]}[kind]
    tails = [ptr(a[t]) for t in _TAILS[:ntail]]
    two = [hws, hws_bytes] if kind in ("seq", "nbest") else []
    st = getattr(lib, entry)(*head, *mid, *tails, ptr(a["grad"]), ws, ws_bytes, *two, None)
    del keep, keep_h
    return st


def replay(lib):
    """({entry: {label: status}}, {query: {label: bytes}}) over the whole grid."""
    statuses = {entry: {label: status(lib, entry, ov) for label, ov in cases(entry)} for entry in ENTRIES}
    sizes = {name: {label: int(getattr(lib, name)(*args)) for label, args in rows} for name, rows in size_cases().items()}
    return statuses, sizes
