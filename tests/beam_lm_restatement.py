"""TEST INFRASTRUCTURE ONLY: CPU restatement (numpy float32) of the LM-fused CTC prefix beam search
that csrc/beam_lm.hip runs on the device, an independent float64 ARPA evaluator with a brute force
over every prefix, and a writer of random ARPA files.

The restatement extends oracle/ctc_beam_oracle.py (same candidate numbering k = w*C + c, stay / merge
/ suppress rules and tie-breaking) by the kernel's LM state and scoring rule, with the kernel's order
of float32 operations:
  word score (delimiter after a non-empty word part): delta = ((sum back-offs + logp) + unk) + beta
  partial-word penalty (ranking only): pen = unk_score_offset * max(1, len/6) for a dead word part
  rank = (tot + acc') + pen
LM values are float32(alpha) * float32(ln10 * log10 value), as the device image stores them. The LM
tables here are plain dictionaries built from the parsed ARPA file, not the hashed device image.
Parity with pyctcdecode itself is unpinned (it is not installed)."""
from __future__ import annotations

import itertools
import math

import numpy as np

from oracle.ctc_beam_oracle import NEG, _lse, log_softmax32

F = np.float32
LN10 = math.log(10.0)


class Tables:
    """Dictionary form of an LM for the restatement: spell (token ids of a word -> word id), prefixes
    (every prefix of a spelled word), ng ((w1..wk) -> (alpha ln p, alpha ln back-off) float32)."""

    def __init__(self, lm, vocab, blank, delim, alpha, beta, unk_score_offset):
        char_id = {t: i for i, t in enumerate(vocab) if len(t) == 1 and i not in (blank, delim)}
        self.spell, self.prefixes = {}, {()}
        for wid, word in enumerate(lm.words):
            if word in ("<s>", "</s>", "<unk>") or any(ch not in char_id for ch in word):
                continue
            ids = tuple(char_id[ch] for ch in word)
            self.spell[ids] = wid
            self.prefixes.update(ids[:i] for i in range(1, len(ids) + 1))
        a = F(alpha)
        self.ng = {ids: (a * F(LN10 * p), a * F(LN10 * bo)) for ids, (p, bo) in lm.ngrams.items()}
        self.order = lm.order
        self.unk, self.bos, self.eos = lm.word_id["<unk>"], lm.word_id.get("<s>", -1), lm.word_id.get("</s>", -1)
        self.beta = F(beta)
        self.unk_offset = F(unk_score_offset)
        self.unk_scaled = a * F(LN10 * unk_score_offset)

    def word_lm(self, hist, w):
        n = min(self.order - 1, len(hist))
        h = hist[len(hist) - n:]
        bo = F(0.0)
        for k in range(n, -1, -1):
            ctx = h[n - k:]
            hit = self.ng.get(ctx + (w,))
            if hit is not None:
                return F(bo + hit[0])
            if k > 0 and ctx in self.ng:
                bo = F(bo + self.ng[ctx][1])
        return bo

    def word_delta(self, part, hist):
        """(delta, word id) of the word part ended after the history."""
        w = self.spell.get(part)
        wid = self.unk if w is None else w
        return F(F(self.word_lm(hist, wid) + (self.unk_scaled if w is None else F(0.0))) + self.beta), wid

    def penalty(self, part):
        if part in self.prefixes:
            return F(0.0)
        return F(self.unk_offset * max(F(1.0), F(F(len(part)) / F(6.0))))


def ctc_prefix_beam_lm(logits, tab, beam, blank=0, delim=4, token_min_logp=-5.0, beam_prune_logp=-10.0,
                       score_boundary=False, length=None):
    """logits (T, C) of one sample -> (token tuple of the best prefix, its CTC log p, its fused score)."""
    logits = np.asarray(logits, np.float32)
    T, C = logits.shape
    T = T if length is None else min(length, T)
    tmin = F(token_min_logp)
    hist0 = (tab.bos,) if score_boundary else ()
    # (prefix, log p_b, log p_nb, word part, word history, LM score), sorted slots
    beams = [((), F(0.0), NEG, (), hist0, F(0.0))]
    for t in range(T):
        y = log_softmax32(logits[t])
        arg = int(np.argmax(y))
        use = [bool(y[c] >= tmin or c == arg) for c in range(C)]
        cand = {}
        tots_b = [_lse(pb, pnb) for _, pb, pnb, *_ in beams]
        for w, (pre, pb, pnb, *_) in enumerate(beams):
            tot = tots_b[w]
            if tot == NEG:
                continue
            last = pre[-1] if pre else -1
            for c in range(C):
                vb, vnb = NEG, NEG
                if c == blank:
                    if use[c]:
                        vb = F(tot + y[blank])
                    if last >= 0 and use[last]:
                        vnb = F(pnb + y[last])
                elif use[c]:
                    vnb = F((pb if c == last else tot) + y[c])
                cand[w * C + c] = [vb, vnb]
        index = {b[0]: w for w, b in enumerate(beams) if tots_b[w] != NEG}
        merged = []
        for w, (pre, *_) in enumerate(beams):
            if not pre or tots_b[w] == NEG or not use[pre[-1]]:
                continue
            w0 = index.get(pre[:-1])
            if w0 is None or w0 == w:
                continue
            ke = w0 * C + pre[-1]
            cand[w * C + blank][1] = _lse(cand[w * C + blank][1], cand[ke][1])
            merged.append(ke)
        for ke in merged:
            cand[ke] = [NEG, NEG]
        # the word each beam's word part ends if the delimiter follows
        ends = {w: tab.word_delta(b[3], b[4]) for w, b in enumerate(beams)
                if b[3] and tots_b[w] != NEG and use[delim]}
        ranks, state = {}, {}
        for k, (vb, vnb) in cand.items():
            tot = _lse(vb, vnb)
            if tot == NEG:
                continue
            w, c = divmod(k, C)
            _, _, _, part, hist, acc = beams[w]
            if c == delim:
                if part:
                    d, wid = ends[w]
                    acc, hist = F(acc + d), (hist + (wid,))[-4:]
                part = ()
            elif c != blank:
                part = part + (c,)
            ranks[k] = F(F(tot + acc) + tab.penalty(part))
            state[k] = (part, hist, acc)
        best = max(ranks.values()) if ranks else NEG
        thr = F(best + F(beam_prune_logp))
        keep = sorted((k for k, v in ranks.items() if v >= thr), key=lambda k: (-ranks[k], k))[:beam]
        nb = []
        for k in keep:
            w, c = divmod(k, C)
            pre = beams[w][0]
            nb.append((pre if c == blank else pre + (c,), cand[k][0], cand[k][1], *state[k]))
        beams = nb
    if not beams or T == 0:
        return (), F(0.0), F(0.0)
    best, out = NEG, None
    for pre, pb, pnb, part, hist, acc in beams:
        tot = _lse(pb, pnb)
        if tot == NEG:
            continue
        if part:
            d, wid = tab.word_delta(part, hist)
            acc, hist = F(acc + d), (hist + (wid,))[-4:]
        if score_boundary:
            acc = F(acc + tab.word_lm(hist, tab.eos))
        rank = F(tot + acc)
        if out is None or rank > best:
            best, out = rank, (pre, tot, rank)
    return out


# ---- independent float64 reference: a dictionary ARPA evaluator and a brute force over prefixes ----

def arpa64(path):
    """{(w1, .., wk) words: (log10 p, log10 back-off)} read straight from the ARPA text."""
    grams = {}
    for line in open(path, encoding="utf-8"):
        p = line.rstrip("\n").split("\t")
        if len(p) >= 2 and not line.startswith("\\"):
            grams[tuple(p[1].split())] = (float(p[0]), float(p[2]) if len(p) > 2 else 0.0)
    grams.setdefault(("<unk>",), (-100.0, 0.0))
    return grams


def log10p64(grams, order, hist, w):
    """log10 p(w | hist) by the back-off recursion p(w | h) = bo(h) * p(w | h[1:])."""
    hist = tuple(hist)[len(hist) - min(order - 1, len(hist)):]
    if hist + (w,) in grams:
        return grams[hist + (w,)][0]
    return grams.get(hist, (0.0, 0.0))[1] + log10p64(grams, order, hist[1:], w)


def lm_score64(grams, order, vocab, prefix, delim, alpha, beta, unk_score_offset, score_boundary):
    """The fused LM score of a token sequence: per word alpha ln p + beta (+ alpha ln10 unk offset for
    a word the LM does not have), plus alpha ln p(</s>) with score_boundary."""
    hist = ["<s>"] if score_boundary else []
    total = 0.0
    parts = [list(g) for is_d, g in itertools.groupby(prefix, lambda c: c == delim) if not is_d]
    for part in parts:
        word = "".join(vocab[c] for c in part)
        known = (word,) in grams and word not in ("<s>", "</s>", "<unk>")
        word = word if known else "<unk>"
        total += alpha * LN10 * log10p64(grams, order, hist, word) + beta
        total += 0.0 if known else alpha * LN10 * unk_score_offset
        hist.append(word)
    if score_boundary:
        total += alpha * LN10 * log10p64(grams, order, hist, "</s>")
    return total


def ctc_logp64(logits, prefix, blank=0):
    """log P_ctc(prefix | logits) by the CTC forward recursion in float64."""
    x = np.asarray(logits, np.float64)
    y = x - x.max(1, keepdims=True)
    y = y - np.log(np.exp(y).sum(1, keepdims=True))
    ext = [blank]
    for c in prefix:
        ext += [c, blank]
    a = np.full(len(ext), -np.inf)
    a[0] = y[0, blank]
    if len(ext) > 1:
        a[1] = y[0, ext[1]]
    for t in range(1, x.shape[0]):
        n = np.full(len(ext), -np.inf)
        for s in range(len(ext)):
            v = [a[s]] + ([a[s - 1]] if s >= 1 else [])
            if s >= 2 and ext[s] != blank and ext[s] != ext[s - 2]:
                v.append(a[s - 2])
            n[s] = np.logaddexp.reduce(v) + y[t, ext[s]]
        a = n
    return float(np.logaddexp.reduce(a[-2:]) if len(ext) > 1 else a[0])


def all_prefixes(T, C, blank=0):
    """Every token sequence of at most T tokens (one with repeats that T frames cannot spell, a
    repeated token needing a blank between, has log P_ctc = -inf)."""
    toks = [c for c in range(C) if c != blank]
    return [p for n in range(T + 1) for p in itertools.product(toks, repeat=n)]


def brute_force64(logits, grams, order, vocab, delim, alpha, beta, unk_score_offset, score_boundary):
    """{prefix: log P_ctc(prefix) + LM(prefix)} in float64 over every prefix."""
    T, C = np.asarray(logits).shape
    return {p: ctc_logp64(logits, p) + lm_score64(grams, order, vocab, p, delim, alpha, beta, unk_score_offset,
                                                  score_boundary) for p in all_prefixes(T, C)}


# ---- random ARPA files ----

def write_random_arpa(path, words, order, n_higher, seed, with_unk=True):
    """An ARPA file over `words` (plus <s>, </s> and, with_unk, <unk>): every unigram, and n_higher
    n-grams of orders 2..order grown by extending an n-gram of the order below with a random word."""
    rng = np.random.default_rng(seed)
    uni = ["<s>", "</s>"] + (["<unk>"] if with_unk else []) + list(words)
    grams = {1: [(w,) for w in uni]}
    per = max(1, n_higher // max(1, order - 1))
    for k in range(2, order + 1):
        seen = set()
        base = [g for g in grams[k - 1] if g[-1] != "</s>"]
        while len(seen) < per:
            g = base[rng.integers(len(base))]
            w = uni[rng.integers(1, len(uni))]       # never <s>
            seen.add(g + (w,))
        grams[k] = sorted(seen)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n" + "".join(f"ngram {k}={len(grams[k])}\n" for k in grams) + "\n")
        for k in grams:
            f.write(f"\\{k}-grams:\n")
            for g in grams[k]:
                p = -rng.uniform(0.3, 4.0)
                bo = "" if k == order or g[-1] == "</s>" else f"\t{-rng.uniform(0.0, 1.0):.4f}"
                f.write(f"{p:.4f}\t{' '.join(g)}{bo}\n")
            f.write("\n")
        f.write("\\end\\\n")
    return path


def random_words(n, letters, seed, max_len=6):
    rng = np.random.default_rng(seed)
    out = set()
    while len(out) < n:
        out.add("".join(letters[i] for i in rng.integers(len(letters), size=rng.integers(1, max_len + 1))))
    return sorted(out)
