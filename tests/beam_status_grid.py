"""The status grid of the eight beam-search entries: which status each returns for which arguments, without a GPU.

Every call has its arrays in HOST memory.  A call that passes the checks has no workspace and stops at PGASR_ERR_WORKSPACE; a call
with a workspace is one the checks refuse (a byte short, the node limit), so no call reaches HIP.  ``cases(entry)`` lists
(label, overrides of ``base(entry)``) and ``status(lib, entry, overrides)`` makes the call; tests/test_beam_status_cpu.py replays
the grid against tests/golden/beam_status_grid.json, which tools/dev/beam_status_record.py writes from another commit's library.
"""
import ctypes

import numpy as np

SIZE_MAX = (1 << 64) - 1

# entry -> (wide, list, lm, bias): which argument groups its signature has
ENTRIES = {
    "pgasr_ctc_beam_search": (False, False, False, False),
    "pgasr_ctc_beam_search_lm": (False, False, True, False),
    "pgasr_ctc_beam_search_nbest": (False, True, True, False),
    "pgasr_ctc_beam_search_bias": (False, False, True, True),
    "pgasr_ctc_beam_search_nbest_bias": (False, True, True, True),
    "pgasr_ctc_beam_search_wide": (True, True, False, False),
    "pgasr_ctc_beam_search_wide_lm": (True, True, True, False),
    "pgasr_ctc_beam_search_wide_bias": (True, True, True, True),
}
NARROW = [e for e, k in ENTRIES.items() if not k[0]]

_DUMMY = np.zeros(1 << 16, dtype=np.uint8)        # what every non-NULL array argument points to: nothing is read before a refusal


def limits(entry):
    """(vmax, kmax, trie nodes) of the entry's kernel: csrc/beam.hip, csrc/beam_wide.hip, TrieWs<SYM_BITS>::MAX_NODES."""
    return (1024, 128, 1 << 22) if ENTRIES[entry][0] else (64, 128, 1 << 24)


def base(entry):
    """Arguments that pass every check the entry makes without a model or a bias table (True / False: an array or NULL)."""
    wide = ENTRIES[entry][0]
    return dict(lp=True, is_f64=0, T=6, B=2, V=70 if wide else 29, beam=4, blank=0, flags=0,
                nbest=3, tok=True, tok_stride=None, tl=True, sc=True, cnt=True,      # tok_stride None: T
                ws=None, lm_table=False, lm_order=0, lm_alpha=0.0, lm_beta=0.0,       # ws: None, "short", "full" or "limit"
                tables=False, tables_states=True, tables_order=2,                     # the wide entries' unit model
                bias_table=False, bias_states=0, bias_weight=0.0)


def _lm_on(entry):
    if ENTRIES[entry][0]:
        return dict(tables=True, lm_alpha=0.5, lm_beta=0.1)
    return dict(lm_table=True, lm_order=2, lm_alpha=0.5, lm_beta=0.1)


_BIAS_ON = dict(bias_table=True, bias_states=4, bias_weight=1.5)
NAN, INF = float("nan"), float("inf")


def _node_limit(entry):
    """(T, beam) with T * beam + 1 == the trie's node limit exactly: the first size that is refused."""
    return (60787, 69) if ENTRIES[entry][0] else (159783, 105)


def cases(entry):
    wide, has_list, has_lm, has_bias = ENTRIES[entry]
    vmax, kmax, nodes = limits(entry)
    V = base(entry)["V"]
    T, beam = _node_limit(entry)
    assert T * beam + 1 == nodes
    one = [{}]
    one += [{p: False} for p in ("lp", "tok", "tl", "sc")]
    one += [{k: v} for k in ("T", "B", "V", "beam") for v in (0, -1)]
    one += [{"blank": -1}, {"blank": V}, {"blank": V - 1}, {"V": vmax + 1}, {"V": vmax}, {"beam": kmax + 1}, {"beam": kmax}, {"is_f64": 1}]
    one += [{"flags": f} for f in list(range(1, 64)) + [64, 128, 1 << 30]]
    one += [{"ws": "short"}, {"ws": "limit", "T": T, "beam": beam}, {"T": T, "beam": beam}]
    if has_list:
        one += [{"nbest": 0}, {"nbest": -1}, {"nbest": 5}, {"nbest": 4}, {"tok_stride": 5}, {"tok_stride": 7}, {"cnt": False}]
    out = [(c, {}) for c in one]
    on = {}
    if has_lm:
        on.update(_lm_on(entry))
        lm = [{}, {"lm_alpha": NAN}, {"lm_alpha": INF}, {"lm_beta": NAN}, {"lm_beta": -INF}]
        if wide:
            lm += [{"tables": False}, {"tables_states": False}, {"tables_order": -1}, {"tables_order": 0}, {"tables_order": 5},
                   {"tables_order": 6}, {"V": 71}, {"blank": 1}]
        else:
            lm += [{"lm_order": -1}, {"lm_order": -1, "lm_table": False}, {"lm_order": 0}, {"lm_table": False}, {"lm_order": 5}, {"lm_order": 6},
                   {"lm_order": 5, "V": 32}, {"lm_order": 5, "V": 33}, {"lm_order": 4, "V": 64}, {"lm_order": 5, "V": 64}]
        out += [(c, _lm_on(entry)) for c in lm]
    if has_bias:
        on.update(_BIAS_ON)
        bias = [{}, {"bias_table": False, "bias_states": 0}, {"bias_table": False}, {"bias_states": 0}, {"bias_states": -3},
                {"bias_states": (1 << 24) // V + 1}, {"bias_states": (1 << 24) // V}, {"bias_weight": NAN}, {"bias_weight": INF},
                {"bias_weight": -INF}, {"bias_weight": 0.0}]
        bias += [{"flags": f} for f in range(1, 64)]
        out += [(c, _BIAS_ON) for c in bias]
    if on:
        out += [(c, on) for c in one]
        # two refusals at once: the order of the checks (the model's, the bias table's, the list's, the workspace)
        two = [{"V": vmax + 1, "lm_alpha": NAN}, {"ws": "limit", "T": T, "beam": beam, "lm_alpha": NAN}]
        lm6 = {"tables_order": 6} if wide else {"lm_order": 6}      # a model that is refused as unsupported
        if wide:
            two += [dict(lm6, flags=2)]
        if has_list:
            two += [dict(lm6, nbest=0)]
        if has_bias:
            two += [dict(lm6, bias_table=False), {"lm_beta": INF, "bias_table": False}]
            if has_list:
                two += [{"flags": 8, "nbest": 0}, {"bias_weight": NAN, "nbest": 0}]
        out += [(c, on) for c in two]
    res = {}
    for change, context in out:
        ov = dict(context, **change)
        res.setdefault(",".join(f"{k}={ov[k]!r}" for k in sorted(ov)) or "base", ov)      # the same call reached twice is one case
    return list(res.items())


def _need(lib, entry, a):
    if not ENTRIES[entry][0]:
        return lib.pgasr_beam_workspace_bytes(a["T"], a["B"], a["V"], a["beam"])
    fn = lib.pgasr_beam_wide_lm_workspace_bytes if a["tables"] else lib.pgasr_beam_wide_workspace_bytes
    return fn(a["T"], a["B"], a["V"], a["beam"])


def status(lib, entry, overrides):
    """The entry's status for base(entry) with ``overrides``."""
    wide, has_list, has_lm, has_bias = ENTRIES[entry]
    a = dict(base(entry), **overrides)
    ptr = lambda on: _DUMMY.ctypes.data if on else None      # noqa: E731
    keep = None
    if a["ws"] is None:
        ws, ws_bytes = None, 0
    elif a["ws"] == "limit":                                  # refused for its size: the pointer is never used
        ws, ws_bytes = _DUMMY.ctypes.data, SIZE_MAX
    else:
        need = _need(lib, entry, a)
        assert 0 < need < 1 << 28
        keep = np.zeros(need, dtype=np.uint8)
        ws, ws_bytes = keep.ctypes.data, need - (a["ws"] == "short")
    args = [ptr(a["lp"]), a["is_f64"], a["B"] * a["V"], a["V"], None, a["T"], a["B"], a["V"], a["beam"], a["blank"], a["flags"]]
    if has_list:
        stride = a["T"] if a["tok_stride"] is None else a["tok_stride"]
        args += [a["nbest"], ptr(a["tok"]), stride, ptr(a["tl"]), ptr(a["sc"]), ptr(a["cnt"])] + ([None] if wide else [])
    else:
        args += [ptr(a["tok"]), ptr(a["tl"]), ptr(a["sc"])]
    args += [ws, ws_bytes, None]
    tables = None
    if has_lm and wide:
        if a["tables"]:
            from policy_gradient_asr_amd import _lib
            V = base(entry)["V"]
            tables = _lib.UnitLMTables()
            tables.states, tables.succ = ptr(a["tables_states"]), ptr(True)
            tables.order, tables.vocab, tables.blank, tables.n_states, tables.n_succ, tables.start = a["tables_order"], V, 0, V + 2, V - 1, 1
        args += [ctypes.byref(tables) if tables is not None else None, a["lm_alpha"], a["lm_beta"]]
    elif has_lm:
        args += [ptr(a["lm_table"]), a["lm_order"], a["lm_alpha"], a["lm_beta"]]
    if has_bias:
        args += [ptr(a["bias_table"]), a["bias_states"], a["bias_weight"]]
    st = getattr(lib, entry)(*args)
    del keep, tables
    return st


def replay(lib):
    """{entry: {label: status}} over the whole grid."""
    return {entry: {label: status(lib, entry, ov) for label, ov in cases(entry)} for entry in ENTRIES}
