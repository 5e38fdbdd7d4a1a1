"""Drop-in for the reference's CTCdecoder.py: ``CTCDecoder(alphabet).decode(probs, beam_size=100,
blank=0) -> (tuple[int], float)`` and ``collapse_fn(str) -> str``, with the search itself running
as a HIP kernel (csrc/beam.hip).  ``greedy_decode`` is the best-path decoder the reference lacks
(SURVEY §8a A9).  Beyond the reference: ``nbest=N`` returns the first N entries of the final beam instead of the best one, and
``CTCDecoder.rescore`` ranks such a list in a second pass (exact CTC likelihood and / or a stronger n-gram LM, csrc/nbest.hip; the
likelihood of lists of more than 16 rows or more than 64 symbols from the lattice-free scorer, csrc/hyp_score.hip; with
``word_lm=`` a word n-gram LM on top, csrc/word_lm.hip; with ``unit_lm=`` a back-off LM over the units themselves, csrc/unit_lm.hip);
``CTCDecoder.mbr_decode`` returns the hypothesis of least expected edit distance under the list's posterior instead of the best-scored
one (minimum-Bayes-risk decoding, csrc/mbr.hip); ``CTCDecoder(hotwords=...)`` biases the search towards a list of phrases (contextual
biasing with a weighted automaton, ``lm.HotwordBias``; csrc/beam.hip BIAS = true) and ``rescore(bias=...)`` applies the same bias to a list
in the second pass (csrc/hotword.hip), which is how lists of subword units get it unless ``wide_hotwords=True`` puts the bias into
the wide search itself (csrc/beam_wide.hip with a WideBias)."""
import collections

import numpy as np
import torch

from . import hipops


def _device(device=None):
    if device is not None:
        return torch.device(device)
    if not torch.cuda.is_available():
        raise RuntimeError("policy_gradient_asr_amd needs the MI355X: there is no CPU decoder")
    return torch.device("cuda", torch.cuda.current_device())


BEAM_KMAX = 128      # csrc/beam.hip


def _check_search_vocab(V):
    """The beam searches hold one symbol per lane; wider rows have the best-path decoder only."""
    if V > hipops.MAX_VOCAB_NARROW:
        raise ValueError(f"the beam search takes at most {hipops.MAX_VOCAB_NARROW} output symbols (got {V}): decode a wider alphabet "
                         f"greedily -- CTCdecoder.greedy_decode, model.predict(beam_size=0) -- which takes up to "
                         f"{hipops.MAX_VOCAB_WIDE}")


_UNSET = object()      # "use the decoder's own value" (None is a value: no language model)

NBestRescored = collections.namedtuple("NBestRescored", "order total am lm_logp best_tokens best_len skipped")
NBestRescoredWords = collections.namedtuple("NBestRescoredWords", NBestRescored._fields + ("word_logp", "n_words", "n_oov"))
NBestRescoredUnits = collections.namedtuple("NBestRescoredUnits", NBestRescored._fields + ("unit_logp",))
NBestRescoredWordsUnits = collections.namedtuple("NBestRescoredWordsUnits", NBestRescoredWords._fields + ("unit_logp",))


def _with_bias(res, bias_score):
    """``res`` with one more field at its end: bias (N,B) float64, B(y) of every hypothesis."""
    cls = collections.namedtuple(type(res).__name__ + "Bias", type(res)._fields + ("bias",))
    return cls(*res, bias_score)
MBRDecoded = collections.namedtuple("MBRDecoded", "tokens lengths best risk posterior dist nbest")


class CTCDecoder:
    def __init__(self, alphabet, device=None, lm=None, lm_alpha=0.0, lm_beta=0.0, fast_lm=False, wide_search=False, unit_lm=None,
                 fused_word_lm=None, fused_word_alpha=0.0, fused_word_beta=0.0, word_delimiter=None, oov_penalty=0.0,
                 wide_hotwords=False, hotwords=None, hotword_weight=1.0):
        """lm: None (default: the acoustic search of the reference) or a ``lm.CharNgramLM``; every extension of a prefix by a
        non-blank symbol s then gets ``lm_alpha * ln p_lm(s | last order-1 symbols) + lm_beta`` added (Hannun/Maas,
        arXiv:1408.2873 -- the place CTCdecoder.py:90-96 marks for an LM score).  ``decode`` / ``decode_batch`` use these values
        unless a call overrides them.
        fast_lm: ``decode_batch`` with an LM takes the single-wave kernel where its limits allow (``hipops.ctc_beam_search``:
        fp32 log-probs, beam_size <= 16, at most 64 symbols, T * beam_size <= 24576, T <= 4096) instead of the several times slower
        workgroup kernel; a call may override it.  ``decode`` is the fp64 drop-in and always takes the exact kernel.
        wide_search: opt in to the exact search over rows of 65 .. 1024 symbols (``hipops.ctc_beam_search_wide``, csrc/beam_wide.hip):
        ``decode`` and ``decode_batch``, the ``nbest=`` forms included, then take that entry for rows of more than 64 symbols.  It has
        no language-model fusion: such rows together with an LM raise.  Rows of at most 64 symbols make the calls they always made;
        with the default False wider rows are refused as before.
        unit_lm: None or a ``lm.UnitNgramLM`` (a sparse back-off model over the units themselves, up to 1024 symbols), fused into the
        wide search with ``lm_alpha`` / ``lm_beta`` as ``lm`` is into the narrow one (``hipops.ctc_beam_search_wide(unit_lm=)``).  It
        needs ``wide_search=True`` and excludes ``lm``; rows of at most 64 symbols then take the wide entry too.  A model whose
        vocabulary or blank differs from a call's raises.
        hotwords: None (default: every call is the call it was) or a ``lm.HotwordBias``, or a list of strings compiled with this
        decoder's alphabet and blank 0 (``HotwordBias.from_strings``): ``decode`` / ``decode_batch`` and their ``nbest=`` forms then add
        ``hotword_weight * bonus`` to every extension on the way into or through a phrase (``hipops.ctc_beam_search(bias=)``), with or
        without ``lm``, and their scores are FUSED scores.  ``set_hotwords(hotwords, weight)`` changes the list later.  The biased
        search is the workgroup kernel's: fast_lm=True with hotwords raises, and so do rows of more than 64 symbols and ``unit_lm`` --
        the wide search takes no bias unless ``wide_hotwords`` is given; without it bias its lists in the second pass,
        ``rescore(bias=)``.  A bias whose vocabulary or blank differs from a call's raises.
        wide_hotwords: with ``wide_search=True`` (ValueError without it), the calls that take the wide entry -- rows of more than 64
        symbols, or any rows once ``unit_lm`` is given; ``decode``, ``decode_batch`` and their ``nbest=`` forms -- pass the hotwords
        there (``hipops.ctc_beam_search_wide(bias=)``, csrc/beam_wide.hip): the first pass itself is biased, with or without
        ``unit_lm``, so a rare phrase stays in the beam instead of having to be in the list already when a second pass looks for it.
        Rows of at most 64 symbols without ``unit_lm`` keep taking the narrow biased kernel.
        fused_word_lm: None (default: every call is the call it was) or a ``lm.WordNgramLM`` -- made a ``lm.WordFusion`` over this
        alphabet with blank 0, ``word_delimiter`` (default the alphabet's " ") and ``oov_penalty`` (<= 0; -inf: only lexicon words) --
        or a ready ``lm.WordFusion`` (``word_delimiter`` and ``oov_penalty`` are then its own).  ``decode`` / ``decode_batch`` and their
        ``nbest=`` forms then take ``hipops.ctc_beam_search_words`` (csrc/beam.hip WORDS = true): the word model and its lexicon act
        inside the first pass -- every word end adds ``fused_word_alpha * ln p(word | history) + fused_word_beta``, the final beam is
        ranked with the pending word and </s> scored -- and the scores are FUSED scores.  Not together with ``lm``, ``hotwords``,
        ``fast_lm``, ``wide_search`` / ``unit_lm`` or more than 64 symbols (ValueError naming the option).  ``rescore(word_lm=)`` stays
        the second pass it is."""
        self.fused_word_lm = None
        self.fused_word_alpha, self.fused_word_beta = float(fused_word_alpha), float(fused_word_beta)
        if fused_word_lm is not None:
            from .lm import WordFusion, WordNgramLM
            for name, given in (("lm", lm is not None), ("hotwords", hotwords is not None), ("fast_lm", bool(fast_lm)),
                                ("wide_search", bool(wide_search)), ("unit_lm", unit_lm is not None)):
                if given:
                    raise ValueError(f"{name}: not together with fused_word_lm -- the word LM is fused into the workgroup kernel's "
                                     f"search, alone")
            if len(alphabet) > hipops.MAX_VOCAB_NARROW:
                raise ValueError(f"fused_word_lm: the fused search takes at most {hipops.MAX_VOCAB_NARROW} symbols (got "
                                 f"{len(alphabet)})")
            if isinstance(fused_word_lm, WordNgramLM):
                self.alphabet = alphabet
                fused_word_lm = WordFusion(fused_word_lm, len(alphabet), self._word_delimiter(word_delimiter), blank=0,
                                           oov_penalty=oov_penalty)
            elif not isinstance(fused_word_lm, WordFusion):
                raise ValueError("fused_word_lm: a lm.WordFusion or a lm.WordNgramLM is wanted")
            for name, x in (("fused_word_alpha", self.fused_word_alpha), ("fused_word_beta", self.fused_word_beta)):
                if x != x or x in (float("inf"), -float("inf")):
                    raise ValueError(f"{name} must be finite")
            self.fused_word_lm = fused_word_lm
        if wide_hotwords and not wide_search:
            raise ValueError("wide_hotwords: the bias is fused into the wide search; give wide_search=True")
        self.wide_hotwords = bool(wide_hotwords)
        if unit_lm is not None and lm is not None:
            raise ValueError("unit_lm: not together with lm -- one first-pass language model")
        if unit_lm is not None and not wide_search:
            raise ValueError("unit_lm: the model is fused into the wide search; give wide_search=True")
        self.unit_lm = unit_lm
        self.alphabet = alphabet
        self.NEG_INF = -float("inf")
        self.device = device
        self.lm, self.lm_alpha, self.lm_beta = lm, float(lm_alpha), float(lm_beta)
        self.fast_lm = bool(fast_lm)
        self.wide_search = bool(wide_search)
        self.hotwords, self.hotword_weight = None, 1.0
        self.set_hotwords(hotwords, hotword_weight)

    def set_hotwords(self, hotwords, weight=1.0):
        """The decoder's hotword list from now on: None, a ``lm.HotwordBias`` or a list of strings (see the constructor)."""
        from .lm import HotwordBias
        if hotwords is not None:
            if self.fused_word_lm is not None:
                raise ValueError("hotwords: not together with fused_word_lm -- the word LM is fused into the search alone")
            if self.fast_lm:
                raise ValueError("fast_lm: the single-wave kernel has no hotword bias; give fast_lm=False with hotwords")
            if self.unit_lm is not None and not self.wide_hotwords:
                raise ValueError("hotwords: the wide search has no hotword bias (unit_lm is fused into it); bias its lists in the "
                                 "second pass, rescore(bias=)")
            if not isinstance(hotwords, HotwordBias):
                if isinstance(hotwords, str):
                    raise ValueError("hotwords: a list of strings or a lm.HotwordBias, not one string")
                hotwords = HotwordBias.from_strings(list(hotwords), self.alphabet, blank=0)
        weight = float(weight)
        if weight != weight or weight in (float("inf"), -float("inf")):
            raise ValueError("hotword_weight must be finite")
        self.hotwords, self.hotword_weight = hotwords, weight

    def _bias_args(self, V, blank, wide, fast_lm=False):
        """The bias keywords of the narrow entries, and of the wide one with ``wide_hotwords``; refuses what no kernel does.
        Touches no device."""
        if self.hotwords is None:
            return {}
        if wide and not self.wide_hotwords:
            raise ValueError(f"hotwords: the wide beam search ({V} symbols) has no hotword bias; bias its lists in the second pass, "
                             f"rescore(bias=)")
        if fast_lm and not wide:
            raise ValueError("fast_lm: the single-wave kernel has no hotword bias; give fast_lm=False with hotwords")
        if self.hotwords.vocab != V or self.hotwords.blank != int(blank):
            raise ValueError(f"hotwords: the bias is over {self.hotwords.vocab} symbols with blank {self.hotwords.blank}; the call has "
                             f"{V} symbols and blank {int(blank)}")
        return {"bias": self.hotwords, "bias_weight": self.hotword_weight}

    def _takes_wide(self, V, args, blank=0):
        """Whether rows of V symbols go to the wide search; refuses what neither search takes.  Touches no device."""
        if self.unit_lm is not None:
            if args["lm"] is not None:
                raise ValueError("unit_lm: not together with lm -- one first-pass language model")
            if V > hipops.MAX_VOCAB_SEARCH_WIDE:
                raise ValueError(f"the wide beam search takes at most {hipops.MAX_VOCAB_SEARCH_WIDE} output symbols (got {V})")
            hipops._unit_lm_check(self.unit_lm, V, blank)
            return True
        if V <= hipops.MAX_VOCAB_NARROW:
            return False
        if not self.wide_search:
            _check_search_vocab(V)
        if V > hipops.MAX_VOCAB_SEARCH_WIDE:
            raise ValueError(f"the wide beam search takes at most {hipops.MAX_VOCAB_SEARCH_WIDE} output symbols (got {V})")
        if args["lm"] is not None:
            raise ValueError(f"lm: the wide beam search ({V} > {hipops.MAX_VOCAB_NARROW} symbols) has no language-model fusion; "
                             f"search without one (lm=None)")
        return True

    def _wide_lm(self, args):
        """The language-model and bias keywords of the wide entry."""
        bias = {k: args[k] for k in ("bias", "bias_weight") if k in args}
        if self.unit_lm is None:
            return bias
        return {"unit_lm": self.unit_lm, "lm_alpha": args["lm_alpha"], "lm_beta": args["lm_beta"], **bias}

    def _fused_check(self, V, blank, args, fast_lm=False):
        """The refusals of a call with ``fused_word_lm``, by option name; no device is touched."""
        f = self.fused_word_lm
        if args["lm"] is not None:
            raise ValueError("lm: not together with fused_word_lm -- the word LM is fused into the search alone; call with lm=None")
        if fast_lm:
            raise ValueError("fast_lm: the single-wave kernel has no word LM fusion; give fast_lm=False with fused_word_lm")
        if V > hipops.MAX_VOCAB_NARROW:
            raise ValueError(f"fused_word_lm: the fused search takes at most {hipops.MAX_VOCAB_NARROW} symbols (got {V})")
        if f.vocab != V or f.blank != int(blank):
            raise ValueError(f"fused_word_lm: the lexicon is over {f.vocab} symbols with blank {f.blank}; the call has {V} symbols and "
                             f"blank {int(blank)}")

    def _fused_search(self, log_probs, lengths, beam_size, blank, args, nbest, fast_lm=False):
        """The call with ``fused_word_lm``: ``hipops.ctc_beam_search_words`` behind ``_fused_check``."""
        self._fused_check(log_probs.shape[-1], blank, args, fast_lm)
        return hipops.ctc_beam_search_words(log_probs, lengths, beam=int(beam_size), nbest=1 if nbest is None else int(nbest),
                                            blank=int(blank), fusion=self.fused_word_lm, alpha=self.fused_word_alpha,
                                            beta=self.fused_word_beta)

    def _lm_args(self, lm, lm_alpha, lm_beta):
        return {"lm": self.lm if lm is _UNSET else lm,
                "lm_alpha": self.lm_alpha if lm_alpha is None else float(lm_alpha),
                "lm_beta": self.lm_beta if lm_beta is None else float(lm_beta)}

    def decode(self, probs, beam_size=100, blank=0, lm=_UNSET, lm_alpha=None, lm_beta=None, nbest=None):
        """probs: (time x output dim) array of PROBABILITIES (CTCdecoder.py:41-53).
        Returns (label tuple, negative log-likelihood of that prefix).  With a language model (the decoder's, or ``lm`` /
        ``lm_alpha`` / ``lm_beta`` given here; ``lm=None`` switches it off for this call) the second value is the FUSED score
        -logsumexp(p_blank, p_nonblank) with the LM bonuses in it, not a negative log-likelihood.
        Limits of the device search (the reference has none): beam_size <= 128 and at most 64 output symbols (1024 with
        ``wide_search=True``, where the language model is the decoder's ``unit_lm`` or none) -- a larger request raises instead of
        silently searching a narrower beam.
        nbest: None (default: the pair above) or N with 1 <= N <= beam_size: a list of (label tuple, score) pairs, the first
        min(N, size of the final beam) entries of the final beam in the search's rank order (best first; equal scores in first-touch
        order, like the reference's sorted(...)[:N])."""
        args = self._lm_args(lm, lm_alpha, lm_beta)
        if self.fused_word_lm is not None:
            T, V = np.shape(probs)
            self._fused_check(V, blank, args)
            if int(beam_size) > BEAM_KMAX:
                raise ValueError(f"beam_size {beam_size} exceeds the device search's limit of {BEAM_KMAX}")
            if T == 0:                                       # the empty prefix, finalised on the host: no device needed
                row = (tuple(), -(0.0 + self.fused_word_lm.final((), self.fused_word_alpha, self.fused_word_beta, True)))
                return row if nbest is None else [row]
            with np.errstate(divide="ignore"):
                logp = np.log(np.asarray(probs).astype(np.float64)).reshape(T, 1, V)
            lp = torch.from_numpy(np.ascontiguousarray(logp)).to(_device(self.device))
            nb = self._fused_search(lp, None, beam_size, blank, args, nbest)
            tok, tl, sc = nb.tokens[:, 0].cpu(), nb.lengths[:, 0].tolist(), nb.score[:, 0].tolist()
            rows = [(tuple(int(x) for x in tok[r, :tl[r]].tolist()), float(sc[r])) for r in range(int(nb.count[0].item()))]
            return rows[0] if nbest is None else rows
        if self.wide_search:                                 # refused before a device is asked for
            self._takes_wide(np.shape(probs)[-1], args, blank)
        if self.hotwords is not None:                        # likewise
            V0 = np.shape(probs)[-1]
            self._bias_args(V0, blank, self._takes_wide(V0, args, blank))
        dev = _device(self.device)
        probs = np.asarray(probs)
        T, V = probs.shape
        wide = self._takes_wide(V, args, blank)
        args.update(self._bias_args(V, blank, wide))
        if T == 0:
            return (tuple(), -0.0) if nbest is None else [(tuple(), -0.0)]
        with np.errstate(divide="ignore"):
            logp = np.log(probs.astype(np.float64))          # like CTCdecoder.py:55
        lp = torch.from_numpy(np.ascontiguousarray(logp)).to(dev).view(T, 1, V)
        if int(beam_size) > BEAM_KMAX:
            raise ValueError(f"beam_size {beam_size} exceeds the device search's limit of {BEAM_KMAX}")
        if nbest is not None:
            if wide:
                nb = hipops.ctc_beam_search_wide(lp, None, beam=int(beam_size), nbest=int(nbest), blank=int(blank), **self._wide_lm(args))
            else:
                nb = hipops.ctc_beam_search_nbest(lp, None, beam=int(beam_size), nbest=int(nbest), blank=int(blank), **args)
            tok, tl, sc = nb.tokens[:, 0].cpu(), nb.lengths[:, 0].tolist(), nb.score[:, 0].tolist()
            return [(tuple(int(x) for x in tok[r, :tl[r]].tolist()), float(sc[r])) for r in range(int(nb.count[0].item()))]
        if wide:
            tokens, tl, score = hipops.ctc_beam_search_wide(lp, None, beam=int(beam_size), blank=int(blank), **self._wide_lm(args))
        else:
            tokens, tl, score = hipops.ctc_beam_search(lp, None, beam=int(beam_size), blank=int(blank), **args)
        n = int(tl[0].item())
        return tuple(int(x) for x in tokens[0, :n].tolist()), float(score[0].item())

    def decode_batch(self, log_probs, lengths=None, beam_size=5, blank=0, lm=_UNSET, lm_alpha=None, lm_beta=None, fast_lm=None,
                     nbest=None):
        """Device-side batched form: log_probs (T,B,V) GPU tensor of natural-log probabilities.
        Returns (tokens (B,T) int32, lengths (B) int32, nll (B) float64) without a host sync.  With a language model (see
        ``decode``) the third value is the fused score, not a negative log-likelihood.
        nbest: None (default: the triple above) or N with 1 <= N <= beam_size: ``hipops.CTCNBest`` (tokens (N,B,T), lengths (N,B),
        score (N,B), count (B)), still without a host sync; see ``hipops.ctc_beam_search_nbest``.
        fast_lm: None (default: the decoder's own) or a bool -- with an LM, take the single-wave kernel where its limits allow."""
        fast_lm = self.fast_lm if fast_lm is None else bool(fast_lm)
        args = self._lm_args(lm, lm_alpha, lm_beta)
        if self.fused_word_lm is not None:
            nb = self._fused_search(log_probs, lengths, beam_size, blank, args, nbest, fast_lm)
            return (nb.tokens[0], nb.lengths[0], nb.score[0]) if nbest is None else nb
        if self.hotwords is not None:
            bias_args = self._bias_args(log_probs.shape[-1], blank, self._takes_wide(log_probs.shape[-1], args, blank), fast_lm)
            args.update(bias_args)
        if self._takes_wide(log_probs.shape[-1], args, blank):
            return hipops.ctc_beam_search_wide(log_probs, lengths, beam=int(beam_size), blank=int(blank),
                                               nbest=None if nbest is None else int(nbest), **self._wide_lm(args))
        if nbest is not None:
            return hipops.ctc_beam_search_nbest(log_probs, lengths, beam=int(beam_size), nbest=int(nbest), blank=int(blank),
                                                fast_lm=fast_lm, **args)
        return hipops.ctc_beam_search(log_probs, lengths, beam=int(beam_size), blank=int(blank), fast_lm=fast_lm, **args)

    def _word_delimiter(self, word_delimiter):
        if word_delimiter is not None:
            return int(word_delimiter)
        for i, sym in enumerate(self.alphabet):
            if sym.replace("\n", "") == " ":
                return i
        raise ValueError("a word LM needs word_delimiter: the alphabet has no ' ' symbol")

    def rescore(self, log_probs, lengths, nb, lm=_UNSET, lm_alpha=None, lm_beta=None, acoustic="ctc", am_weight=1.0, max_hyp_len=None,
                blank=0, word_lm=None, word_lm_alpha=0.0, word_lm_beta=0.0, word_delimiter=None, scorer=None, unit_lm=None,
                unit_lm_alpha=0.0, unit_lm_beta=0.0, bias=None, bias_weight=0.0):
        """Second pass over an N-best list ``nb`` (``hipops.CTCNBest`` of ``decode_batch(..., nbest=N)`` on the same log_probs
        (T,B,V) / lengths), N <= 128:  total = am_weight * am - lm_alpha * lm_logp - lm_beta * length, lower is better, with
        lm_logp the hypothesis' log-probability under ``lm`` (the decoder's own unless given; None: no LM term).
        acoustic="ctc" (default): am = -log p(y|x) over ALL alignments of the hypothesis (``hipops.ctc_hyp_lattice`` on fp32
            log-probs), not the search's partial sum.  The lattices are sized by Lh = hyp_len_cap(T, max_hyp_len); with
            max_hyp_len=None the longest hypothesis of the list is read from the device -- ONE host synchronisation, which keeps the
            lattice workspace at the size the list needs instead of T.  Give max_hyp_len to avoid it.  A hypothesis longer than
            Lh is not scored: it is marked in ``skipped`` and gets total = +inf.
        acoustic="first_pass": am = nb.score, no synchronisation.  After a search fused with an LM that score already contains
            the first pass' LM bonuses: the second LM is then added on top of them, not in their place.
        Returns ``NBestRescored``: order (B,N) int32 -- per utterance the list's rows by ascending total, ties in first-pass order,
        rows beyond count last --, total / am / lm_logp (N,B) float64, best_tokens (B,T) / best_len (B) int32 the row order[:, 0]
        of every utterance, skipped (N,B) bool.
        word_lm: None (default: everything above, nothing else) or a ``lm.WordNgramLM``.  The pass above runs first and its total
            is the base of a second launch: total = base - word_lm_alpha * word_logp - word_lm_beta * n_words, with word_logp the
            log-probability of the hypothesis' words under ``word_lm`` (``hipops.nbest_word_lm_score``; words split at the token
            ``word_delimiter``, default the alphabet's " " -- an alphabet without one raises).  Returns ``NBestRescoredWords``:
            the seven fields above with order / total / best_* from the combined total, then word_logp (N,B) float64, n_words and
            n_oov (N,B) int32.  No further host synchronisation.  word_lm_alpha = word_lm_beta = 0 leaves order and total as
            they are without a word LM, bit for bit.
        scorer: what computes am for acoustic="ctc".  "lattice": ``hipops.ctc_hyp_lattice`` (fp32 nll, both sweeps of every pair in
            a workspace; at most 64 symbols and N <= 16, else ValueError).  "forward": ``hipops.ctc_hyp_score`` (csrc/hyp_score.hip:
            the forward sweep alone, fp64, no workspace; up to 1024 symbols, N <= 128), am = +inf where skipped.  None (default):
            the lattice within its limits -- the call made before the forward scorer existed, the same bits in every field --, the
            forward scorer beyond them.
        Lists over more than 64 symbols (``CTCDecoder(wide_search=True)``): ``lm`` and ``word_lm`` must be None (ValueError naming
            the option: a subword unit may span a space and the character tables hold 64 symbols); total = am_weight * am - lm_beta *
            length and its rank come from ``hipops.nbest_combine_rank`` -- the formula above without an LM, with the same roundings --
            and lm_logp is zeros.
        unit_lm: None (default: everything above, nothing else) or a ``lm.UnitNgramLM`` over the list's V symbols and ``blank`` -- the
            language model of wide lists, and of narrow ones alike.  The pass above runs first and its total is the base of one more
            launch pair: total = base - unit_lm_alpha * unit_logp - unit_lm_beta * length, with unit_logp the hypothesis'
            ``logp_sequence`` (``hipops.nbest_unit_lm_score``) and the roundings of the formula above
            (``hipops.nbest_combine_rank``); a word LM, if any, comes on top of that.  The result carries one more field, unit_logp
            (N,B) float64 (``NBestRescoredUnits`` / ``NBestRescoredWordsUnits``).  No further host synchronisation.
        bias: None (default: everything above, nothing else) or a ``lm.HotwordBias`` over the list's V symbols and ``blank`` -- narrow
            and wide lists alike, which is how lists of subword units are biased.  It comes last: total = total - bias_weight * B(y),
            with B(y) the hypothesis' ``score_sequence`` (``hipops.nbest_bias_score``) and the roundings of
            ``hipops.nbest_combine_rank`` on the earlier total.  The result carries one more field at its end, bias (N,B) float64
            (the result's type with "Bias" behind its name).  No further host synchronisation.  With acoustic="first_pass" after a
            search that was itself biased -- the narrow one, or the wide one of ``CTCDecoder(wide_hotwords=True)`` --, am already
            holds the first pass' bonuses: the bias is then added on top of them.  acoustic="ctc" drops them: am is the exact
            likelihood of every row, and the biased first pass has only decided which rows are in the list."""
        if unit_lm is not None:
            hipops._unit_lm_check(unit_lm, log_probs.shape[-1], blank)
        if bias is not None:
            from .lm import HotwordBias
            if not isinstance(bias, HotwordBias):
                raise ValueError("bias: a lm.HotwordBias is wanted (never raw tensors)")
            if bias.vocab != log_probs.shape[-1] or bias.blank != int(blank):
                raise ValueError(f"bias: the hotwords are over {bias.vocab} symbols with blank {bias.blank}; the list has "
                                 f"{log_probs.shape[-1]} symbols and blank {int(blank)}")
        if acoustic not in ("ctc", "first_pass"):
            raise ValueError(f"acoustic must be 'ctc' or 'first_pass' (got {acoustic!r})")
        if scorer not in (None, "lattice", "forward"):
            raise ValueError(f"scorer must be None, 'lattice' or 'forward' (got {scorer!r})")
        T, B, V = log_probs.shape
        N = nb.tokens.shape[0]
        args = self._lm_args(lm, lm_alpha, lm_beta)
        wide = V > hipops.MAX_VOCAB_NARROW
        if wide:
            for name, given in (("lm", args["lm"] is not None), ("word_lm", word_lm is not None)):
                if given:
                    raise ValueError(f"{name}: not over a list of {V} > {hipops.MAX_VOCAB_NARROW} symbols -- a subword unit may span a "
                                     f"space and the n-gram tables hold characters; rescore such a list with {name}=None")
        in_lattice_limits = not wide and N <= hipops.MAX_SAMPLES
        if scorer == "lattice" and not in_lattice_limits:
            raise ValueError(f"scorer='lattice' takes at most {hipops.MAX_VOCAB_NARROW} symbols and {hipops.MAX_SAMPLES} hypotheses per "
                             f"utterance (got {V} and {N}): take scorer='forward'")
        forward = scorer == "forward" or (scorer is None and not in_lattice_limits)
        if word_lm is not None:
            delim = self._word_delimiter(word_delimiter)
            if nb.tokens.shape[2] > hipops.WORD_LM_MAX_STRIDE:
                raise ValueError(f"a word LM takes hypotheses of at most {hipops.WORD_LM_MAX_STRIDE} tokens (got rows of "
                                 f"{nb.tokens.shape[2]})")
        if acoustic == "ctc":
            if lengths is None:
                lengths = torch.full((B,), T, dtype=torch.int32, device=log_probs.device)
            Lh = hipops.hyp_len_cap(T, int(nb.lengths.max().item()) if max_hyp_len is None else max_hyp_len)
            skipped = nb.lengths > Lh
            if forward:
                am = hipops.ctc_hyp_score(log_probs.float().contiguous(), nb.tokens, nb.lengths, lengths.to(torch.int32).contiguous(),
                                          Lh, count=nb.count, blank=int(blank))
            else:
                nll, _ = hipops.ctc_hyp_lattice(log_probs.float().contiguous(), nb.tokens, nb.lengths,
                                                lengths.to(torch.int32).contiguous(), Lh, blank=int(blank))
                am = torch.where(skipped, torch.full_like(nb.score, float("inf")), nll.double())
        else:
            skipped = torch.zeros_like(nb.lengths, dtype=torch.bool)
            am = nb.score
        if wide:
            # pgasr_nbest_rescore's total without an LM, ((am_weight * am) + -0) + -(lm_beta * length), each rounded once
            order, total = hipops.nbest_combine_rank((am * float(am_weight)).contiguous(), torch.zeros_like(am),
                                                     nb.lengths.clamp(0, nb.tokens.shape[2]), nb.count, word_alpha=0.0,
                                                     word_beta=args["lm_beta"])
            lm_logp = torch.zeros_like(am)
        else:
            order, total, lm_logp = hipops.nbest_rescore(nb.tokens, nb.lengths, nb.count, am.contiguous(), V, blank=int(blank),
                                                         lm=args["lm"], am_weight=float(am_weight), lm_alpha=args["lm_alpha"],
                                                         lm_beta=args["lm_beta"])
        if unit_lm is not None:
            unit_logp = hipops.nbest_unit_lm_score(nb.tokens, nb.lengths, nb.count, unit_lm)
            order, total = hipops.nbest_combine_rank(total, unit_logp, nb.lengths.clamp(0, nb.tokens.shape[2]), nb.count,
                                                     word_alpha=float(unit_lm_alpha), word_beta=float(unit_lm_beta))
        if word_lm is not None:
            word_logp, n_words, n_oov = hipops.nbest_word_lm_score(nb.tokens, nb.lengths, nb.count, word_lm, delim)
            order, total = hipops.nbest_combine_rank(total, word_logp, n_words, nb.count, word_alpha=float(word_lm_alpha),
                                                     word_beta=float(word_lm_beta))
        if bias is not None:
            bias_score = hipops.nbest_bias_score(nb.tokens, nb.lengths, nb.count, bias)
            order, total = hipops.nbest_combine_rank(total, bias_score, torch.zeros_like(nb.lengths), nb.count,
                                                     word_alpha=float(bias_weight), word_beta=0.0)
        first = order[:, 0].long()
        cols = torch.arange(B, device=order.device)
        best = (nb.tokens[first, cols].contiguous(), nb.lengths[first, cols].contiguous())
        if word_lm is not None:
            res = NBestRescoredWords(order, total, am, lm_logp, best[0], best[1], skipped, word_logp, n_words, n_oov)
            res = res if unit_lm is None else NBestRescoredWordsUnits(*res, unit_logp)
        else:
            res = NBestRescored(order, total, am, lm_logp, best[0], best[1], skipped)
            res = res if unit_lm is None else NBestRescoredUnits(*res, unit_logp)
        return res if bias is None else _with_bias(res, bias_score)

    def mbr_from_list(self, nb, score, vocab=None, risk_unit="char", word_delimiter=None, posterior_scale=1.0, max_hyp_len=None,
                      unit_spelling=None):
        """Minimum-Bayes-risk choice over an N-best list the caller already holds: ``nb`` a ``hipops.CTCNBest`` (N <= 128), ``score``
        (N,B) float64 with lower better (``rescore(...).total``, ``nb.score``, ...), ``vocab`` the number of symbols (default: the
        alphabet's).  posterior = softmax(-posterior_scale * score) over the list's valid rows; the row of least expected edit
        distance to the others under it is returned (the first among equals).
        risk_unit: "char" (default: the list's own units -- characters, or the subword units of a wide alphabet --,
            ``hipops.nbest_pair_distance`` on the bit-vector kernel for at most 64 symbols and on the wave-per-pair kernels above) or
            "word" (words split at the token ``word_delimiter``, the alphabet's " ", as str.split(" ") cuts them; at most 64
            symbols, ValueError above: a subword unit may span a space).
        max_hyp_len: None reads the longest hypothesis from the device for risk_unit="char" (ONE host synchronisation); a number
            avoids it, and a hypothesis longer than that takes no part (risk +inf, posterior 0).
        Returns ``MBRDecoded``: tokens (B,T) / lengths (B) int32 the chosen row of every utterance, best (B) int32 its rank in the
        list, risk (N,B) / posterior (N,B) float64, dist (B,N,N) int32 (-1 where a row takes no part), nbest = ``nb``.
        risk[best[b], b] is the expected number of unit (word) errors of the returned hypothesis: a confidence.
        unit_spelling: None (default: everything above) or the ``units.UnitSpelling`` of a list of subword units: the distances come
            from the spelled text of the list (``hipops.nbest_pair_distance_spelled``) -- risk_unit="char" its characters, "word" its
            words, split at the spelling's " " (no word_delimiter), whatever the number of units; max_hyp_len then caps the spelled
            rows.  The returned tokens stay the list's unit rows."""
        if risk_unit not in ("char", "word"):
            raise ValueError(f"risk_unit must be 'char' or 'word' (got {risk_unit!r})")
        V = len(self.alphabet) if vocab is None else int(vocab)
        if unit_spelling is not None:
            if word_delimiter is not None:
                raise ValueError("unit_spelling brings its own word delimiter, the id of ' ' in the spelled text: give no word_delimiter")
            if unit_spelling.vocab != V:
                raise ValueError(f"unit_spelling spells {unit_spelling.vocab} symbols (units and blank), the list is over {V}")
            dist = hipops.nbest_pair_distance_spelled(nb.tokens, nb.lengths, nb.count, unit_spelling, max_hyp_len=max_hyp_len,
                                                      unit=risk_unit)
        else:
            dist = hipops.nbest_pair_distance(nb.tokens, nb.lengths, nb.count, V, max_hyp_len=max_hyp_len, unit=risk_unit,
                                              delimiter=word_delimiter)
        best, risk, posterior = hipops.mbr_select(dist, score.contiguous(), nb.count, scale=float(posterior_scale))
        first = best.long()
        cols = torch.arange(first.numel(), device=first.device)
        return MBRDecoded(nb.tokens[first, cols].contiguous(), nb.lengths[first, cols].contiguous(), best, risk, posterior, dist, nb)

    def mbr_decode(self, log_probs, lengths=None, beam_size=16, nbest=16, risk_unit="char", word_delimiter=None, acoustic="ctc",
                   posterior_scale=1.0, lm=_UNSET, lm_alpha=None, lm_beta=None, am_weight=1.0, max_hyp_len=None, blank=0,
                   word_lm=None, word_lm_alpha=0.0, word_lm_beta=0.0, unit_lm=None, unit_lm_alpha=0.0, unit_lm_beta=0.0,
                   unit_spelling=None, bias=None, bias_weight=0.0):
        """Minimum-Bayes-risk decoding: the N-best search (``decode_batch(nbest=)``, with the decoder's first-pass LM if it has
        one), the score of every hypothesis (``rescore(...).total`` with ``acoustic`` / ``lm`` / ``lm_alpha`` / ``lm_beta`` /
        ``am_weight`` as ``rescore`` takes them: without an LM the exact CTC -log p, or the first-pass score), the distances inside
        each list and the selection (``mbr_from_list``), in that order.  log_probs (T,B,V) GPU tensor, nbest <= beam_size, nbest <= 128.
        word_lm / word_lm_alpha / word_lm_beta go to ``rescore`` (words split at ``word_delimiter``, as the word risk): the
        posterior then comes from the totals with the word LM in them; unit_lm / unit_lm_alpha / unit_lm_beta likewise (a
        ``lm.UnitNgramLM`` in the second pass, wide lists included).  unit_spelling: the risk over the spelled text of a list of
        subword units (``mbr_from_list``; max_hyp_len keeps capping the unit rows, the spelled rows by that many units' longest
        spelling).  bias / bias_weight go to ``rescore`` (a ``lm.HotwordBias`` in the second pass); the decoder's own hotwords bias the
        N-best search itself, the wide one with ``wide_hotwords=True``, and acoustic="first_pass" keeps their bonuses in the scores.
        Returns ``MBRDecoded``."""
        T, B, V = log_probs.shape
        nb = self.decode_batch(log_probs, lengths, beam_size=beam_size, blank=blank, nbest=int(nbest))
        rs = self.rescore(log_probs, lengths, nb, lm=lm, lm_alpha=lm_alpha, lm_beta=lm_beta, acoustic=acoustic, am_weight=am_weight,
                          max_hyp_len=max_hyp_len, blank=blank, word_lm=word_lm, word_lm_alpha=word_lm_alpha,
                          word_lm_beta=word_lm_beta, word_delimiter=word_delimiter, unit_lm=unit_lm, unit_lm_alpha=unit_lm_alpha,
                          unit_lm_beta=unit_lm_beta, **({} if bias is None else {"bias": bias, "bias_weight": bias_weight}))
        if unit_spelling is not None:
            cap = None if max_hyp_len is None else int(max_hyp_len) * unit_spelling.max_unit_chars
            return self.mbr_from_list(nb, rs.total, vocab=V, risk_unit=risk_unit, word_delimiter=word_delimiter,
                                      posterior_scale=posterior_scale, max_hyp_len=cap, unit_spelling=unit_spelling)
        return self.mbr_from_list(nb, rs.total, vocab=V, risk_unit=risk_unit, word_delimiter=word_delimiter,
                                  posterior_scale=posterior_scale, max_hyp_len=max_hyp_len)

    def confidence(self, md, pivot="mbr", unit="char", word_delimiter=None, max_hyp_len=None):
        """N-best confidences of a decoded hypothesis (``hipops.nbest_confidence``; Wessel et al. 2001): ``md`` an ``MBRDecoded``
        (``mbr_decode`` / ``mbr_from_list``), whose list is aligned to the pivot row and weighted with ``md.posterior``.
        pivot: "mbr" (default: ``md.best``, the row ``md.tokens`` holds), "map" (row 0, the best-scored one) or a (B) int tensor of
        ranks.  unit: "char" (the list's own units) or "word" (words split at ``word_delimiter``, default the alphabet's " "; at
        most 64 symbols, ValueError above: a subword unit may hold a space).
        Returns ``hipops.NBestConfidence``: per position of the pivot row the posterior mass of the hypotheses whose canonical
        alignment (diagonal, then deletion, then insertion on the walk back) has a hit there, the masses that substitute or drop
        it, and per gap the expected number of extra symbols.  No host synchronisation."""
        nb = md.nbest
        B = nb.tokens.shape[1]
        if isinstance(pivot, str):
            if pivot not in ("mbr", "map"):
                raise ValueError(f"pivot must be 'mbr', 'map' or a tensor of ranks (got {pivot!r})")
            piv = md.best if pivot == "mbr" else torch.zeros(B, dtype=torch.int32, device=nb.tokens.device)
        else:
            piv = torch.as_tensor(pivot, device=nb.tokens.device).to(torch.int32).reshape(-1)
            if piv.numel() != B:
                raise ValueError(f"pivot: one rank per utterance is wanted ({B}), got {piv.numel()}")
        if unit not in ("char", "word"):
            raise ValueError(f"unit must be 'char' or 'word' (got {unit!r})")
        delim = None
        if unit == "word":
            if len(self.alphabet) > hipops.MAX_VOCAB_NARROW:
                raise ValueError(f"unit='word': not over {len(self.alphabet)} > {hipops.MAX_VOCAB_NARROW} symbols -- a subword unit may "
                                 f"hold a space; take unit='char' (the units are the symbols)")
            delim = self._word_delimiter(word_delimiter)
        return hipops.nbest_confidence(nb.tokens, nb.lengths, nb.count, md.posterior.contiguous(), piv.contiguous(), unit=unit,
                                       delimiter=delim, max_hyp_len=max_hyp_len, vocab=len(self.alphabet))

    def decode_words(self, log_probs, lengths=None, beam_size=16, nbest=16, pivot="map", posterior_scale=1.0, word_delimiter=None,
                     **scoring):
        """Words with time stamps and confidences: ``mbr_decode`` (``scoring``: its scoring keywords -- acoustic, lm, lm_alpha,
        lm_beta, am_weight, word_lm, ..., max_hyp_len, blank), ``confidence`` at character and at word level against the pivot row
        ("map": row 0, "mbr": the row of least risk), and ``align_batch`` of the pivot rows.  Alphabets of at most 64 symbols
        with a " " (or ``word_delimiter``).  Returns, per utterance, a list of
        ``(word, start_frame, end_frame, confidence, [character confidences])`` -- words as str.split(" ") cuts the row, an empty
        word included with span (-1, -1) and its own confidence; spans from ``word_spans`` (first frame of the first character,
        one past the last frame of the last; (-1, -1) where the row does not fit the frames).  Copies the results to the host."""
        if pivot not in ("map", "mbr"):
            raise ValueError(f"pivot must be 'map' or 'mbr' (got {pivot!r})")
        for name in ("risk_unit", "unit_spelling"):
            if name in scoring:
                raise ValueError(f"{name}: decode_words scores characters and words of the list itself; not a keyword here")
        delim = self._word_delimiter(word_delimiter)
        blank = int(scoring.get("blank", 0))
        md = self.mbr_decode(log_probs, lengths, beam_size=beam_size, nbest=nbest, posterior_scale=posterior_scale,
                             word_delimiter=delim, **scoring)
        return self.words_of_list(md, log_probs, lengths, pivot=pivot, word_delimiter=delim, blank=blank,
                                  max_hyp_len=scoring.get("max_hyp_len"))[0]

    def words_of_list(self, md, log_probs, lengths=None, pivot="map", word_delimiter=None, blank=0, max_hyp_len=None):
        """``decode_words`` behind the search, for a list the caller already holds: ``md`` an ``MBRDecoded`` over ``log_probs``
        (T,B,V) / ``lengths``, ``pivot`` as ``confidence`` takes it.  Returns (words, character confidences, word confidences):
        the per-utterance word lists of ``decode_words`` and the two ``hipops.NBestConfidence`` they were read from."""
        delim = self._word_delimiter(word_delimiter)
        cc = self.confidence(md, pivot=pivot, unit="char", max_hyp_len=max_hyp_len)
        wc = self.confidence(md, pivot=pivot, unit="word", word_delimiter=delim, max_hyp_len=max_hyp_len)
        Lmax = min(cc.tokens.shape[1], hipops.ALIGN_MAX_TOKENS)
        al = self.align_batch(log_probs, cc.tokens[:, :Lmax].contiguous(), cc.lengths.clamp(max=Lmax), lengths, blank=blank)
        tok, tl = cc.tokens.cpu(), cc.lengths.cpu().tolist()
        cconf, wconf = cc.conf.cpu(), wc.conf.cpu()
        st, en = al.token_start.cpu(), al.token_end.cpu()
        out = []
        for b in range(tok.shape[0]):
            n = min(int(tl[b]), Lmax)
            row = [int(k) for k in tok[b, :n]]
            spans = word_spans(st[b, :n].tolist(), en[b, :n].tolist(), row, delim)
            words, first = [], 0
            for w, (s0, s1) in enumerate(spans):
                last = first
                while last < n and row[last] != delim:
                    last += 1
                text = "".join(self.alphabet[k].replace("\n", "") for k in row[first:last])
                words.append((text, s0, s1, float(wconf[b, w]), [float(x) for x in cconf[b, first:last]]))
                first = last + 1
            out.append(words)
        return out, cc, wc

    def align_batch(self, log_probs, tokens, token_lengths, lengths=None, blank=0):
        """Forced alignment on the device: log_probs (T,B,V) fp32 GPU tensor of natural-log probabilities, tokens (B,Lmax) /
        token_lengths (B) int32 the transcripts (Lmax <= 1023).  Returns ``hipops.CTCAlignment`` (score, frame_label, frame_token,
        token_start, token_end, token_logp) without a host sync: the best single alignment of each transcript (Viterbi), its
        negative log-probability (+inf where the transcript does not fit the frames) and the frames each token occupies."""
        T, B, _ = log_probs.shape
        if lengths is None:
            lengths = torch.full((B,), T, dtype=torch.int32, device=log_probs.device)
        return hipops.ctc_forced_align(log_probs, tokens, lengths.to(torch.int32).contiguous(), token_lengths, blank=int(blank))

    def align(self, probs, labels, blank=0):
        """Single-utterance host form: probs (time x output dim) array of PROBABILITIES as ``decode`` takes them, labels a sequence
        of symbol indices, each in range and not blank (else ValueError, before the device is touched).
        Returns (frame_label tuple, [(start, end, mean_log_prob)] per label, score): the label of every frame on the best
        alignment, each label's first and one-past-last frame with the mean log-probability of its frames, and the alignment's
        negative log-probability.  When the labels do not fit the frames the score is +inf, the frame labels are -1 and every
        span is (-1, -1, -inf)."""
        probs = np.asarray(probs)
        T, V = probs.shape
        labels = [int(x) for x in labels]
        blank = int(blank)
        if not 0 <= blank < V:
            raise ValueError(f"blank {blank} outside [0, {V})")
        for i, x in enumerate(labels):
            if not 0 <= x < V or x == blank:
                raise ValueError(f"label {x} at position {i} is blank or outside [0, {V})")
        if len(labels) > hipops.ALIGN_MAX_TOKENS:
            raise ValueError(f"{len(labels)} labels exceed the device alignment's limit of {hipops.ALIGN_MAX_TOKENS}")
        none = [(-1, -1, -float("inf"))] * len(labels)
        if T == 0:
            return tuple(), none, (0.0 if not labels else float("inf"))
        dev = _device(self.device)
        with np.errstate(divide="ignore"):
            logp = np.log(probs.astype(np.float64)).astype(np.float32)
        lp = torch.from_numpy(np.ascontiguousarray(logp)).to(dev).view(T, 1, V)
        tok = torch.tensor([labels or [0]], dtype=torch.int32, device=dev)
        tl = torch.tensor([len(labels)], dtype=torch.int32, device=dev)
        a = self.align_batch(lp, tok, tl, blank=blank)
        score = float(a.score[0].item())
        if score == float("inf"):
            return (-1,) * T, none, score
        st, en, sm = a.token_start[0].tolist(), a.token_end[0].tolist(), a.token_logp[0].tolist()
        spans = [(st[i], en[i], sm[i] / (en[i] - st[i])) for i in range(len(labels))]
        return tuple(a.frame_label[0].tolist()), spans, score


def word_spans(token_start, token_end, tokens, delimiter):
    """Character spans -> word spans, pure host: token_start / token_end / tokens are equally long sequences (one utterance, real
    length only), ``delimiter`` the token that separates words.  Words follow ``str.split(" ")`` as the word reward does: n
    delimiters give n + 1 words, empty ones included.  Returns one (start, end) per word: the first frame of its first
    character and the one-past-last frame of its last; (-1, -1) for an empty word or one with an unaligned character."""
    token_start, token_end, tokens = list(token_start), list(token_end), list(tokens)
    if not len(token_start) == len(token_end) == len(tokens):
        raise ValueError("word_spans: token_start, token_end and tokens must be equally long")
    words, cur = [], []
    for i, k in enumerate(tokens):
        if int(k) == int(delimiter):
            words.append(cur); cur = []
        else:
            cur.append(i)
    words.append(cur)
    out = []
    for w in words:
        if not w or any(int(token_start[i]) < 0 or int(token_end[i]) < 0 for i in w):
            out.append((-1, -1))
        else:
            out.append((int(token_start[w[0]]), int(token_end[w[-1]])))
    return out


def collapse_fn(preds):
    """Remove adjacent duplicate characters of an already-decoded string (CTCdecoder.py:119-131):
    'aabbcc' -> 'abc', '' -> ''.  Pure host string work."""
    out = []
    for ch in preds:
        if not out or ch != out[-1]:
            out.append(ch)
    return "".join(out)


def greedy_decode(scores, lengths=None, blank=0):
    """Best-path decode on the device: scores (T,B,V) GPU tensor (logits or log-probs) ->
    (tokens (B,T) int32, token_lengths (B) int32): argmax per frame (first max wins), collapse
    repeats, drop blank.  Rows of up to hipops.MAX_VOCAB_WIDE = 1024 scores (above 64 the arg-max is the wide kernel)."""
    T, B, V = scores.shape
    if lengths is None:
        lengths = torch.full((B,), T, dtype=torch.int32, device=scores.device)
    greedy, _ = hipops.frame_argmax_sample(scores.contiguous().float(), want_sample=False)
    tokens, tl = hipops.ctc_collapse(greedy[None].contiguous(), lengths.to(torch.int32).contiguous(), blank=blank)
    return tokens[0], tl[0]
