"""Word-level back-off n-gram language model for the LM-fused CTC beam search (csrc/beam_lm.hip).

The reference's test evaluator decodes with pyctcdecode + KenLM (src/train/evaluator.py:148-154,
189-210). Here the LM is an ARPA text file on disk: read_arpa() parses it, build_image() turns it
and the tokenizer's token strings into two open-addressing hash tables (a character trie over the
LM's words and the n-gram table), DeviceNgramLM holds them on the device with the values scaled by
alpha.

Fingerprints. A key is a sequence of small integers ((node, token id) for the trie, the word ids
w1 .. wk for an n-gram); its 64-bit fingerprint is a chain of splitmix64 finalisers from a seed,
fp = step(...step(step(seed, v1), v2)..., vk). The builder checks that all fingerprints of a table
are distinct and nonzero (0 marks an empty slot) and draws another seed if not, so a fingerprint
match on the device is an exact match. Slot = fp & (capacity - 1), linear probing, load <= 0.5.

Values. The device holds float32 natural-log values already multiplied by alpha:
float32(alpha) * float32(ln10 * log10 value), one float32 multiply per entry, done by torch when the
image is moved to the device or alpha changes. The kernel only adds.
"""
from __future__ import annotations

import gzip
import math
from dataclasses import dataclass, field

import numpy as np

MAX_ORDER = 5
LN10 = math.log(10.0)
UNK_LOG10 = -100.0          # KenLM's score of <unk> when the model has none
DEAD = -1                   # trie: no word has this prefix
_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


def _mix64(x: int) -> int:
    x &= _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def fp_step(h: int, v: int) -> int:
    """One link of the fingerprint chain (the kernel's fp_step)."""
    return _mix64(((h ^ ((v + 1) & 0xFFFFFFFF)) + _GOLD) & _M64)


def fingerprint(seed: int, values) -> int:
    h = seed
    for v in values:
        h = fp_step(h, int(v))
    return h


def _mix64_np(x):
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def _fingerprints_np(seed: int, cols: np.ndarray) -> np.ndarray:
    """fingerprint() of every row of cols (n, k) int64."""
    h = np.full(cols.shape[0], seed, dtype=np.uint64)
    for j in range(cols.shape[1]):
        v = ((cols[:, j] + 1) & 0xFFFFFFFF).astype(np.uint64)
        h = _mix64_np((h ^ v) + np.uint64(_GOLD))
    return h


@dataclass
class ArpaLM:
    """A parsed ARPA file. words: id -> word (in order of appearance in the unigram section, <unk>
    appended if the file has none); ngrams: (w1 .. wk) ids -> (log10 p, log10 back-off)."""
    order: int
    counts: list
    words: list
    ngrams: dict
    word_id: dict = field(default_factory=dict)

    def id_of(self, word: str) -> int:
        return self.word_id.get(word, self.word_id["<unk>"])

    def log10_prob(self, context, word: str) -> float:
        """log10 p(word | context words) by the back-off walk (float64; unknown words are <unk>)."""
        w = self.id_of(word)
        h = tuple(self.id_of(x) for x in context)[-(self.order - 1):] if self.order > 1 else ()
        bo = 0.0
        for k in range(len(h), -1, -1):
            ctx = h[len(h) - k:]
            hit = self.ngrams.get(ctx + (w,))
            if hit is not None:
                return bo + hit[0]
            if k > 0 and ctx in self.ngrams:
                bo += self.ngrams[ctx][1]
        raise KeyError(word)   # unreachable: every word id has a unigram


def read_arpa(path: str) -> ArpaLM:
    """Parses an ARPA back-off LM (plain text or .gz), orders 1 to 5."""
    opener = gzip.open if str(path).endswith(".gz") else open
    counts: dict = {}
    words: list = []
    word_id: dict = {}
    ngrams: dict = {}
    section = None          # None: before \data\; 0: in \data\; k: in \k-grams:
    with opener(path, "rt", encoding="utf-8") as f:
        for ln, raw in enumerate(f, 1):
            line = raw.strip()
            if not line:
                continue
            if line == "\\data\\":
                section = 0
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                section = int(line[1:-len("-grams:")])
                if section not in counts:
                    raise ValueError(f"{path}:{ln}: section {line} has no count in \\data\\")
                continue
            if section is None:
                continue
            if section == 0:
                if line.startswith("ngram "):
                    k, n = line[len("ngram "):].split("=")
                    k = int(k)
                    if not 1 <= k <= MAX_ORDER:
                        raise ValueError(f"{path}: n-gram order {k} is not supported (orders 1 to {MAX_ORDER})")
                    counts[k] = int(n)
                continue
            parts = line.split("\t") if "\t" in line else line.split()
            if "\t" in line:
                toks = parts[1].split()
                bo = float(parts[2]) if len(parts) > 2 and parts[2].strip() else 0.0
            else:
                toks = parts[1:1 + section]
                bo = float(parts[1 + section]) if len(parts) > 1 + section else 0.0
            if len(toks) != section:
                raise ValueError(f"{path}:{ln}: expected {section} words, got {len(toks)}")
            if section == 1:
                if toks[0] in word_id:
                    raise ValueError(f"{path}:{ln}: duplicate unigram {toks[0]!r}")
                word_id[toks[0]] = len(words)
                words.append(toks[0])
            try:
                ids = tuple(word_id[t] for t in toks)
            except KeyError as e:
                raise ValueError(f"{path}:{ln}: word {e.args[0]!r} has no unigram") from None
            ngrams[ids] = (float(parts[0]), bo)
    if not counts:
        raise ValueError(f"{path}: no \\data\\ section")
    order = max(counts)
    if sorted(counts) != list(range(1, order + 1)):
        raise ValueError(f"{path}: \\data\\ must list every order from 1 to {order}")
    if "<unk>" not in word_id:
        word_id["<unk>"] = len(words)
        words.append("<unk>")
        ngrams[(word_id["<unk>"],)] = (UNK_LOG10, 0.0)
    return ArpaLM(order, [counts[k] for k in range(1, order + 1)], words, ngrams, word_id)


def _capacity(n: int) -> int:
    cap = 2
    while cap < 2 * n:
        cap <<= 1
    return cap


def _fill_table(fps: np.ndarray, cap: int) -> np.ndarray:
    """slot of every fingerprint under linear probing into cap (power of two) slots: a key lands on
    the first slot from its home that is free when it gets there."""
    mask = cap - 1
    slot_of = np.full(fps.shape[0], -1, dtype=np.int64)
    used = np.zeros(cap, dtype=bool)
    pending = np.arange(fps.shape[0])
    pos = (fps & np.uint64(mask)).astype(np.int64)
    while pending.size:
        free = ~used[pos]
        # of the keys standing on one free slot the first takes it
        _, first = np.unique(pos[free], return_index=True)
        win = np.flatnonzero(free)[first]
        slot_of[pending[win]] = pos[win]
        used[pos[win]] = True
        keep = np.ones(pending.size, dtype=bool)
        keep[win] = False
        pending, pos = pending[keep], (pos[keep] + 1) & mask
    return slot_of


@dataclass
class NgramImage:
    """The host form of the device image (numpy). The lookups below restate the kernel's probing."""
    order: int
    unk_id: int
    bos_id: int              # <s>, -1 if the LM has none
    eos_id: int              # </s>, -1 if the LM has none
    blank: int
    delim: int
    trie_seed: int
    trie_keys: np.ndarray    # uint64 [trie_cap], 0 = empty
    trie_child: np.ndarray   # int32 [trie_cap]
    node_word: np.ndarray    # int32 [nodes], -1 = ends no word
    ng_seed: int
    ng_keys: np.ndarray      # uint64 [ng_cap], 0 = empty
    ng_log10: np.ndarray     # float64 [ng_cap, 2]: log10 p, log10 back-off

    def child(self, node: int, char: int) -> int:
        if node == DEAD:
            return DEAD
        f = fingerprint(self.trie_seed, (node, char))
        mask = len(self.trie_keys) - 1
        s = f & mask
        for _ in range(mask + 1):
            k = int(self.trie_keys[s])
            if k == f:
                return int(self.trie_child[s])
            if k == 0:
                return DEAD
            s = (s + 1) & mask
        return DEAD

    def word_of(self, node: int) -> int:
        return DEAD if node == DEAD else int(self.node_word[node])

    def slot(self, ids) -> int:
        """Table slot of the n-gram (w1 .. wk), -1 if absent."""
        f = fingerprint(self.ng_seed, ids)
        mask = len(self.ng_keys) - 1
        s = f & mask
        for _ in range(mask + 1):
            k = int(self.ng_keys[s])
            if k == f:
                return s
            if k == 0:
                return -1
            s = (s + 1) & mask
        return -1

    def lookup(self, ids):
        """(log10 p, log10 back-off) of the n-gram, None if absent."""
        s = self.slot(ids)
        return None if s < 0 else (float(self.ng_log10[s, 0]), float(self.ng_log10[s, 1]))


def _seeded(build, what: str):
    for attempt in range(16):
        seed = _mix64(0x5EED0000 + attempt) | 1
        out = build(seed)
        if out is not None:
            return seed, out
    raise RuntimeError(f"no seed gave distinct 64-bit fingerprints for the {what}")


def _distinct(fps: np.ndarray) -> bool:
    return bool((fps != 0).all()) and np.unique(fps).size == fps.size


def build_image(lm: ArpaLM, vocab, blank: int = 0, delim: int = 4) -> NgramImage:
    """vocab: token strings by id (datasets.tokenizer.vocab_of). Words are spelled with the
    single-character tokens; a word with a character outside them, or with the blank or the delimiter,
    cannot be produced by the search and is left out of the trie (it stays in the n-gram table)."""
    char_id = {t: i for i, t in enumerate(vocab) if len(t) == 1 and i not in (blank, delim)}
    special = {"<s>", "</s>", "<unk>"}
    edges: dict = {}            # (node, char) -> child
    node_word = [DEAD]
    for wid, word in enumerate(lm.words):
        if word in special or not word or any(ch not in char_id for ch in word):
            continue
        node = 0
        for ch in word:
            key = (node, char_id[ch])
            nxt = edges.get(key)
            if nxt is None:
                nxt = edges[key] = len(node_word)
                node_word.append(DEAD)
            node = nxt
        node_word[node] = wid
    ekeys = np.array(list(edges.keys()), dtype=np.int64).reshape(-1, 2)
    evals = np.array(list(edges.values()), dtype=np.int32)

    def trie_fps(seed):
        fps = _fingerprints_np(seed, ekeys)
        return fps if _distinct(fps) else None
    trie_seed, tf = _seeded(trie_fps, "trie")
    tcap = _capacity(len(tf))
    trie_keys = np.zeros(tcap, dtype=np.uint64)
    trie_child = np.full(tcap, DEAD, dtype=np.int32)
    ts = _fill_table(tf, tcap)
    trie_keys[ts] = tf
    trie_child[ts] = evals

    by_len = [[] for _ in range(lm.order + 1)]
    for ids in lm.ngrams:
        by_len[len(ids)].append(ids)

    def ng_fps(seed):
        fps = np.concatenate([_fingerprints_np(seed, np.array(g, dtype=np.int64).reshape(-1, k))
                              for k, g in enumerate(by_len) if g])
        return fps if _distinct(fps) else None
    ng_seed, gf = _seeded(ng_fps, "n-gram table")
    vals = np.array([lm.ngrams[ids] for g in by_len for ids in g], dtype=np.float64).reshape(-1, 2)
    gcap = _capacity(len(gf))
    ng_keys = np.zeros(gcap, dtype=np.uint64)
    ng_log10 = np.zeros((gcap, 2), dtype=np.float64)
    gs = _fill_table(gf, gcap)
    ng_keys[gs] = gf
    ng_log10[gs] = vals
    return NgramImage(lm.order, lm.word_id["<unk>"], lm.word_id.get("<s>", -1), lm.word_id.get("</s>", -1),
                      blank, delim, trie_seed, trie_keys, trie_child, np.array(node_word, dtype=np.int32),
                      ng_seed, ng_keys, ng_log10)


def scale32(alpha: float, log10_value: float) -> np.float32:
    """The device's value of a log10 score: float32(alpha) * float32(ln10 * log10 value)."""
    return np.float32(alpha) * np.float32(LN10 * log10_value)


class DeviceNgramLM:
    """An NgramImage on a device, with the LM weight alpha folded into the stored values and the word
    insertion bonus beta beside them (functional.ctc_prefix_beam_lm reads both from here)."""

    def __init__(self, image: NgramImage, alpha: float = 0.5, beta: float = 1.5, device="cuda"):
        import torch
        self.image = image
        self.device = torch.device(device)
        # torch has no uint64 arithmetic, and needs none: the keys travel as their int64 bit patterns
        self.trie_keys = torch.from_numpy(image.trie_keys.view(np.int64)).to(self.device)
        self.trie_child = torch.from_numpy(image.trie_child).to(self.device)
        self.node_word = torch.from_numpy(image.node_word).to(self.device)
        self.ng_keys = torch.from_numpy(image.ng_keys.view(np.int64)).to(self.device)
        self._ln = torch.from_numpy(LN10 * image.ng_log10).to(torch.float32).to(self.device)
        self.device = self.ng_keys.device      # "cuda" resolved to the current device's index
        self.beta = float(beta)
        self.set_alpha(alpha)

    def set_alpha(self, alpha: float) -> None:
        import torch
        self.alpha = float(alpha)
        self.ng_vals = (self._ln * torch.tensor(self.alpha, dtype=torch.float32, device=self.device)).contiguous()

    @classmethod
    def from_arpa(cls, path: str, vocab, blank: int = 0, delim: int = 4, alpha: float = 0.5, beta: float = 1.5,
                  device="cuda") -> "DeviceNgramLM":
        return cls(build_image(read_arpa(path), vocab, blank, delim), alpha, beta, device)
