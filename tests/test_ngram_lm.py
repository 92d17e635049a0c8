"""CPU checks of the n-gram LM decode (wav2vec2forbrain_amd/util/ngram_lm.py, csrc/beam_lm.hip's
argument validation, the evaluator and the experiment arguments): the ARPA reader against hand
computed answers, the hashed device image against the parser, and the float32 restatement of the
LM-fused beam search (tests/beam_lm_restatement.py) against a float64 brute force over every prefix
with an independent dictionary ARPA evaluator."""
import ctypes
import gzip
import os

import numpy as np
import pytest

from tests import beam_lm_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = os.path.join(ROOT, "tests", "golden", "tiny_lm.arpa")
VOCAB = ["<pad>", "<s>", "</s>", "<unk>", "|", "E", "T", "A", "O", "N", "I", "H", "S", "R", "D", "L", "U", "M",
         "W", "C", "F", "G", "Y", "P", "B", "V", "K", "'", "X", "J", "Q", "Z"]


def test_read_arpa_known_answers(tmp_path):
    from wav2vec2forbrain_amd.util.ngram_lm import read_arpa
    lm = read_arpa(TINY)
    assert lm.order == 3 and lm.counts == [14, 9, 4]
    assert len(lm.ngrams) == 14 + 9 + 4 + 1                       # + the default <unk>
    assert lm.log10_prob(["THE", "CAT"], "SAT") == -0.2           # a trigram hit
    # back-off through two levels: bo(CAT SAT) + bo(SAT) + p(MAT) = -0.1 - 0.2 - 1.5
    assert lm.log10_prob(["CAT", "SAT"], "MAT") == pytest.approx(-1.8, abs=1e-12)
    assert lm.ngrams[(lm.word_id["AT"],)] == (-2.0, 0.0)          # a missing back-off column is 0
    assert lm.ngrams[(lm.word_id["<unk>"],)] == (-100.0, 0.0)     # absent <unk>: the KenLM convention
    assert lm.log10_prob([], "NOSUCHWORD") == -100.0
    for w in ("<s>", "</s>", "<unk>"):
        assert lm.words[lm.word_id[w]] == w                       # ordinary word ids
    gz = tmp_path / "tiny.arpa.gz"
    with open(TINY, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    assert read_arpa(str(gz)).ngrams == lm.ngrams


def test_read_arpa_rejects_order_6(tmp_path):
    from wav2vec2forbrain_amd.util.ngram_lm import read_arpa
    p = tmp_path / "six.arpa"
    p.write_text("\\data\\\n" + "".join(f"ngram {k}=1\n" for k in range(1, 7)) + "\n\\1-grams:\n-1.0\tA\n\\end\\\n")
    with pytest.raises(ValueError, match="order 6"):
        read_arpa(str(p))


def _check_image(lm, vocab, blank, delim, rng, n_absent=2000):
    from wav2vec2forbrain_amd.util.ngram_lm import DEAD, build_image
    im = build_image(lm, vocab, blank, delim)
    for tab in (im.trie_keys, im.ng_keys):
        used = int((tab != 0).sum())
        assert 2 * used <= len(tab) and len(tab) & (len(tab) - 1) == 0          # load <= 0.5, power of two
        assert np.unique(tab[tab != 0]).size == used                            # distinct fingerprints
    for ids, val in lm.ngrams.items():
        assert im.lookup(ids) == val, ids
    n_words = len(lm.words)
    for _ in range(n_absent):
        ids = tuple(int(v) for v in rng.integers(n_words, size=rng.integers(1, lm.order + 1)))
        assert im.lookup(ids) == lm.ngrams.get(ids)
    assert im.lookup((n_words + 7,)) is None
    # the trie spells every reachable word and nothing else
    chars = {t: i for i, t in enumerate(vocab) if len(t) == 1 and i not in (blank, delim)}
    reach = {w for w in lm.words if w not in ("<s>", "</s>", "<unk>") and all(c in chars for c in w)}
    for w in reach:
        node = 0
        for c in w:
            node = im.child(node, chars[c])
            assert node != DEAD, w
        assert im.word_of(node) == lm.word_id[w]
    ended = [int(v) for v in im.node_word if v >= 0]
    assert sorted(ended) == sorted(lm.word_id[w] for w in reach)
    assert im.child(0, blank) == DEAD and im.child(0, delim) == DEAD and im.child(DEAD, 5) == DEAD
    # probing happened: some key does not sit on its home slot
    moved = lambda tab: any(int(k) & (len(tab) - 1) != s for s, k in enumerate(tab) if k)
    return im, moved(im.trie_keys) or moved(im.ng_keys)


def test_device_image_tiny_lm():
    from wav2vec2forbrain_amd.util.ngram_lm import DEAD, read_arpa
    lm = read_arpa(TINY)
    im, _ = _check_image(lm, VOCAB, 0, 4, np.random.default_rng(0))
    assert lm.word_id["né"] not in im.node_word                   # spelled outside the vocabulary: unreachable
    node = 0
    for c in "IT'S":
        node = im.child(node, VOCAB.index(c))
    assert im.word_of(node) == lm.word_id["IT'S"]
    assert im.word_of(im.child(0, VOCAB.index("C"))) == DEAD      # "C" is a prefix, not a word
    assert im.child(0, 1) == DEAD and im.child(0, 3) == DEAD      # ids 1-3 are letters without edges


def test_device_image_random_lm_probes(tmp_path):
    from wav2vec2forbrain_amd.util.ngram_lm import read_arpa
    words = R.random_words(5000, VOCAB[5:], seed=1)
    path = R.write_random_arpa(str(tmp_path / "big.arpa"), words, 3, 15000, seed=2)
    lm = read_arpa(path)
    assert len(lm.words) == 5003 and len(lm.ngrams) == 5003 + 15000
    _, probed = _check_image(lm, VOCAB, 0, 4, np.random.default_rng(3))
    assert probed


BRUTE_VOCAB = ["_", "|", "A", "B"]


def brute_lm(tmp_path, C):
    letters = BRUTE_VOCAB[2:C]
    words = sorted({"A", "AA"} | ({"AB", "B", "BA"} if C > 3 else set()))
    assert all(set(w) <= set(letters) for w in words)
    return R.write_random_arpa(str(tmp_path / f"brute{C}.arpa"), words, 3, 12 if C > 3 else 8, seed=40 + C)


def check_against_brute_force(decode, path, C, T, seed, boundary, alpha=0.5, beta=0.5, unk=-10.0):
    """decode(logits) -> (prefix, ctc log p, fused score). Criterion of the issue: the returned prefix's
    float64 score is within tolerance of the maximum over all prefixes, and the returned score within
    tolerance of that prefix's float64 score; tolerance 1e-4 * max(1, |ref|)."""
    logits = np.random.default_rng(seed).normal(size=(T, C)).astype(np.float32) * 2.0
    grams = R.arpa64(path)
    ref = R.brute_force64(logits, grams, 3, BRUTE_VOCAB[:C], 1, alpha, beta, unk, boundary)
    assert len(ref) == {(3, 6): 127, (4, 4): 121}[(C, T)]
    pre, ctc, fused = decode(logits)
    best = max(ref.values())
    tol = lambda r: 1e-4 * max(1.0, abs(r))
    print(f"C {C} T {T} seed {seed} boundary {boundary}: prefix {pre} fused {float(fused):.6f} "
          f"float64 of it {ref[tuple(pre)]:.6f} maximum {best:.6f}")
    assert abs(ref[tuple(pre)] - best) <= tol(best), (pre, ref[tuple(pre)], best)
    assert abs(float(fused) - ref[tuple(pre)]) <= tol(ref[tuple(pre)]), (pre, fused, ref[tuple(pre)])
    ctc_ref = R.ctc_logp64(logits, tuple(pre))
    assert abs(float(ctc) - ctc_ref) <= tol(ctc_ref), (pre, ctc, ctc_ref)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("C,T", [(3, 6), (4, 4)])
def test_restatement_matches_float64_brute_force(tmp_path, C, T, seed, boundary):
    from wav2vec2forbrain_amd.util.ngram_lm import read_arpa
    path = brute_lm(tmp_path, C)
    tab = R.Tables(read_arpa(path), BRUTE_VOCAB[:C], 0, 1, 0.5, 0.5, -10.0)

    def decode(logits):
        return R.ctc_prefix_beam_lm(logits, tab, 10 ** 6, 0, 1, -1e30, -1e30, boundary)
    check_against_brute_force(decode, path, C, T, seed, boundary)


def test_capi_argument_validation_without_device():
    from wav2vec2forbrain_amd import _lib
    lib = _lib.load()
    assert lib.b2p_ctc_beam_lm_workspace(2, 10, 16) == 2 * 10 * 16
    one = ctypes.c_void_p(16)          # a non-NULL pointer that is never dereferenced: validation fails first

    def call(order=3, C=32, beam=16, blank=0, delim=4, prune=-10.0, lm_null=False, logits=one, tcap=64):
        d = _lib.NgramLM(16, 16, 16, 16, 16, tcap, 64, 1, 1, order, 2, 0, 1, 0.5, 0)
        _lib.call("b2p_ctc_prefix_beam_lm", logits, 1, 10, C, None, beam, blank, delim, -5.0, prune,
                  None if lm_null else ctypes.byref(d), -10.0, -11.5, 0, one, one, one, one, one, None)
    for bad in (dict(order=0), dict(order=6), dict(C=65), dict(beam=129), dict(beam=0), dict(delim=0),
                dict(delim=32), dict(blank=32), dict(prune=1.0), dict(lm_null=True), dict(logits=None),
                dict(tcap=48)):
        with pytest.raises(RuntimeError, match="ctc_prefix_beam_lm"):
            call(**bad)


def test_evaluator_without_arpa_path_still_raises():
    from wav2vec2forbrain_amd.datasets.tokenizer import create_ctc_tokenizer
    from wav2vec2forbrain_amd.train.evaluator import EvaluatorWithW2vLMDecoder
    tok = create_ctc_tokenizer()
    with pytest.raises(NotImplementedError, match="lm_decode_arpa_path"):
        EvaluatorWithW2vLMDecoder(tok, "test", lm_decode_test_predictions=True)
    EvaluatorWithW2vLMDecoder(tok, "val", lm_decode_test_predictions=True)          # only test mode decodes
    ev = EvaluatorWithW2vLMDecoder(tok, "test", lm_decode_test_predictions=True, lm_decode_arpa_path=TINY)
    assert ev.lm_image is not None and ev.lm_image.order == 3


@pytest.mark.parametrize("module,cls", [("b2t_gru_w2v_experiment", "B2TGruAndW2VArgsModel"),
                                        ("b2t_gru_w2v_conformer_experiment", "B2TGruAndW2VConformerArgsModel")])
def test_new_arguments_parse_with_defaults(module, cls):
    import argparse
    import importlib
    from wav2vec2forbrain_amd.args.argparsing import _parser_from_model
    model = getattr(importlib.import_module(f"wav2vec2forbrain_amd.experiments.{module}"), cls)
    assert model.model_fields["lm_decode_arpa_path"].default is None
    assert model.model_fields["lm_decode_unk_score_offset"].default == -10.0
    parser = _parser_from_model(argparse.ArgumentParser(), model)
    ns = parser.parse_args([])
    assert ns.lm_decode_arpa_path is None and ns.lm_decode_unk_score_offset == -10.0
    ns = parser.parse_args(["--lm_decode_arpa_path", "lm.arpa.gz", "--lm_decode_unk_score_offset", "-7.5"])
    assert ns.lm_decode_arpa_path == "lm.arpa.gz" and ns.lm_decode_unk_score_offset == -7.5
