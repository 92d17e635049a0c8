"""LM-fused CTC prefix beam search on the device (csrc/beam_lm.hip, functional.ctc_prefix_beam_lm)
against the LM-free search it extends (csrc/beam.hip), its float32 restatement
(tests/beam_lm_restatement.py), a float64 brute force over every prefix, and through the evaluator.
The LMs are random ARPA files written per session and the hand-written tests/golden/tiny_lm.arpa.
Parity with pyctcdecode itself is unpinned (it is not installed)."""
import json

import numpy as np
import pytest
import torch

from tests import beam_lm_restatement as R
from tests.test_ngram_lm import BRUTE_VOCAB, TINY, VOCAB, brute_lm, check_against_brute_force

pytestmark = pytest.mark.gpu

ALPHA, BETA, UNK = 0.5, 0.5, -10.0
LENS = [50, 47, 31, 50, 1, 0]


@pytest.fixture(scope="module")
def lms(tmp_path_factory):
    """name -> parsed random LM: 40 short words of order 3, 5,000 words of order 3, 60 words of order 5."""
    from wav2vec2forbrain_amd.util.ngram_lm import read_arpa
    d = tmp_path_factory.mktemp("lms")
    spec = {"small": (R.random_words(40, VOCAB[5:], 7, max_len=3), 3, 120, 8),
            "big": (R.random_words(5000, VOCAB[5:], 1), 3, 15000, 2),
            "order5": (R.random_words(60, VOCAB[5:], 9, max_len=2), 5, 400, 10)}
    return {k: read_arpa(R.write_random_arpa(str(d / f"{k}.arpa"), w, o, n, s)) for k, (w, o, n, s) in spec.items()}


@pytest.fixture(scope="module")
def images(lms):
    from wav2vec2forbrain_amd.util.ngram_lm import build_image
    return {k: build_image(lm, VOCAB, 0, 4) for k, lm in lms.items()}


def _logits():
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(6, 50, 32, generator=g) * 2.5
    logits[:, :, 0] += 2.0            # blank-heavy, as CTC outputs are
    return logits, torch.tensor(LENS, dtype=torch.int32)


def _close(got, ref):
    return abs(float(got) - float(ref)) <= 1e-4 * max(1.0, abs(float(ref)))


@pytest.mark.parametrize("beam", [16, 1])
def test_lm_off_equals_lm_free_search(images, beam):
    """alpha = beta = unk_score_offset = 0, no boundary score: the fused search is the LM-free search,
    bit for bit (tokens, lengths, CTC log p)."""
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util.ngram_lm import DeviceNgramLM
    logits, lens = _logits()
    lm = DeviceNgramLM(images["small"], 0.0, 0.0, "cuda")
    tok, n, ctc, fused = Fn.ctc_prefix_beam_lm(logits.cuda(), lens.cuda(), lm, beam=beam, unk_score_offset=0.0)
    tok0, n0, score0 = Fn.ctc_prefix_beam(logits.cuda(), lens.cuda(), beam=beam)
    assert torch.equal(tok, tok0) and torch.equal(n, n0)
    assert torch.equal(ctc.view(torch.int32), score0.view(torch.int32))
    assert torch.equal(fused, ctc)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("tmin,prune", [(-5.0, -10.0), (-1e30, -1e30)])
@pytest.mark.parametrize("beam", [16, 100])
@pytest.mark.parametrize("name", ["small", "big", "order5"])
def test_device_equals_restatement(lms, images, name, beam, tmin, prune, boundary):
    """Same tokens as the float32 restatement; both scores within 1e-4 * max(1, |ref|)."""
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util.ngram_lm import DeviceNgramLM
    logits, lens = _logits()
    lm = DeviceNgramLM(images[name], ALPHA, BETA, "cuda")
    tok, n, ctc, fused = Fn.ctc_prefix_beam_lm(logits.cuda(), lens.cuda(), lm, beam=beam, token_min_logp=tmin,
                                               beam_prune_logp=prune, unk_score_offset=UNK, score_boundary=boundary)
    tok, n, ctc, fused = tok.cpu().numpy(), n.cpu().numpy(), ctc.cpu().numpy(), fused.cpu().numpy()
    tab = R.Tables(lms[name], VOCAB, 0, 4, ALPHA, BETA, UNK)
    for b in range(len(LENS)):
        ref, ref_ctc, ref_fused = R.ctc_prefix_beam_lm(logits[b].numpy(), tab, beam, 0, 4, tmin, prune, boundary,
                                                       LENS[b])
        assert tuple(tok[b, :n[b]]) == ref, (b, tok[b, :n[b]], ref)
        assert (tok[b, n[b]:] == -1).all()
        assert _close(ctc[b], ref_ctc), (b, ctc[b], ref_ctc)
        assert _close(fused[b], ref_fused), (b, fused[b], ref_fused)


@pytest.mark.parametrize("boundary", [False, True])
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("C,T", [(3, 6), (4, 4)])
def test_device_matches_float64_brute_force(tmp_path, C, T, seed, boundary):
    """W = 128 holds every prefix of these shapes (127 and 121) and nothing is pruned, so the device's
    answer is the float64 maximum of log P_ctc(prefix) + LM(prefix) over all prefixes."""
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util.ngram_lm import DeviceNgramLM, build_image, read_arpa
    path = brute_lm(tmp_path, C)
    lm = DeviceNgramLM(build_image(read_arpa(path), BRUTE_VOCAB[:C], 0, 1), ALPHA, BETA, "cuda")

    def decode(logits):
        tok, n, ctc, fused = Fn.ctc_prefix_beam_lm(torch.from_numpy(logits)[None].cuda(), None, lm, beam=128, blank=0,
                                                   delim=1, token_min_logp=-1e30, beam_prune_logp=-1e30,
                                                   unk_score_offset=UNK, score_boundary=boundary)
        return tuple(int(v) for v in tok[0, :int(n[0])].cpu()), float(ctc[0]), float(fused[0])
    check_against_brute_force(decode, path, C, T, seed, boundary)


def test_lm_changes_the_answer():
    """Frames spell C, then a frame slightly in favour of O over A, then T: the LM-free search returns
    COT, which tests/golden/tiny_lm.arpa does not have; the fused search returns its word CAT."""
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util.ngram_lm import DeviceNgramLM
    ix = VOCAB.index
    logits = torch.full((1, 5, 32), -12.0)
    for t, c in ((0, ix("C")), (1, 0), (3, 0), (4, ix("T"))):
        logits[0, t, c] = 8.0
    logits[0, 2, ix("O")], logits[0, 2, ix("A")] = float(np.log(0.55)), float(np.log(0.45))
    tok, n, _ = Fn.ctc_prefix_beam(logits.cuda(), beam=16)
    assert [VOCAB[c] for c in tok[0, :int(n[0])].cpu()] == list("COT")
    lm = DeviceNgramLM.from_arpa(TINY, VOCAB, alpha=ALPHA, beta=BETA, device="cuda")
    tok, n, ctc, fused = Fn.ctc_prefix_beam_lm(logits.cuda(), None, lm, beam=16)
    assert [VOCAB[c] for c in tok[0, :int(n[0])].cpu()] == list("CAT")
    # fused = log p_ctc + alpha * ln10 * log10 p(CAT) + beta, CAT's unigram being -1.1
    assert _close(fused[0], float(ctc[0]) + ALPHA * np.log(10.0) * -1.1 + BETA)


def test_production_settings(lms, images):
    """The reference's test decoding settings: beam 100, T' = 249 frames, B = 8, the 32-token
    vocabulary, ragged lengths, pyctcdecode's pruning constants, the 5,000-word LM. Two samples against
    the restatement; the device time per batch of the fused and of the LM-free search on the same
    logits is printed, not asserted: nobody has a bound for the cost of the LM."""
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.util.ngram_lm import DeviceNgramLM
    g = torch.Generator().manual_seed(11)
    B, T, C = 8, 249, 32
    logits = torch.randn(B, T, C, generator=g) * 2.5
    logits[:, :, 0] += 2.0
    lens = torch.tensor([249, 249, 240, 200, 249, 131, 249, 64], dtype=torch.int32)
    lm = DeviceNgramLM(images["big"], ALPHA, BETA, "cuda")
    lg, ln = logits.cuda(), lens.cuda()
    tok, n, ctc, fused = Fn.ctc_prefix_beam_lm(lg, ln, lm, beam=100, unk_score_offset=UNK, score_boundary=True)
    tok, n, ctc, fused = tok.cpu().numpy(), n.cpu().numpy(), ctc.cpu().numpy(), fused.cpu().numpy()
    tab = R.Tables(lms["big"], VOCAB, 0, 4, ALPHA, BETA, UNK)
    for b in (0, 5):
        ref, ref_ctc, ref_fused = R.ctc_prefix_beam_lm(logits[b].numpy(), tab, 100, 0, 4, -5.0, -10.0, True,
                                                       int(lens[b]))
        assert tuple(tok[b, :n[b]]) == ref, (b, tok[b, :n[b]], ref)
        assert _close(ctc[b], ref_ctc) and _close(fused[b], ref_fused), (b, ctc[b], ref_ctc, fused[b], ref_fused)
    ms = {}
    for what, run in (("fused", lambda: Fn.ctc_prefix_beam_lm(lg, ln, lm, beam=100, unk_score_offset=UNK,
                                                              score_boundary=True)),
                      ("LM-free", lambda: Fn.ctc_prefix_beam(lg, ln, beam=100))):
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms[what] = e0.elapsed_time(e1) / 5
    print(f"ctc_prefix_beam_lm beam 100 T 249 C 32 B 8, 5,000-word order-3 LM: fused {ms['fused']:.3f} ms, "
          f"LM-free {ms['LM-free']:.3f} ms per batch, ratio {ms['fused'] / ms['LM-free']:.2f}")


def test_evaluator_end_to_end(tmp_path):
    """Test mode with an ARPA path and logits on the GPU: both LM metrics equal the host computation
    from functional.ctc_prefix_beam_lm's tokens, predictions_lm_decoded is kept and reaches the history
    dictionary, and the greedy metrics are what they are without the LM."""
    from transformers import Wav2Vec2CTCTokenizer
    from wav2vec2forbrain_amd import functional as Fn
    from wav2vec2forbrain_amd.datasets.batch_types import B2tSampleBatch
    from wav2vec2forbrain_amd.model.b2tmodel import ModelOutput
    from wav2vec2forbrain_amd.train.evaluator import (EvaluatorWithW2vLMDecoder, char_error_rate, cut_after_eos_token,
                                                       word_error_rate)
    from wav2vec2forbrain_amd.util.ngram_lm import DeviceNgramLM
    f = tmp_path / "vocab.json"
    f.write_text(json.dumps({t: i for i, t in enumerate(VOCAB)}))
    tok = Wav2Vec2CTCTokenizer(str(f))
    g = torch.Generator().manual_seed(21)
    B, T, C, S = 3, 40, 32, 12
    logits = torch.randn(B, T, C, generator=g) * 2.5
    logits[:, :, 0] += 2.0
    lens = torch.tensor([40, 33, 40], dtype=torch.int32)
    target = torch.randint(4, C, (B, S), generator=g)
    sample = B2tSampleBatch(torch.zeros(B, 1, 1).cuda(), target.cuda())

    def run(**kw):
        ev = EvaluatorWithW2vLMDecoder(tok, "test", lm_decode_beam_width=32, lm_decode_alpha=ALPHA,
                                       lm_decode_beta=BETA, lm_decode_score_boundary=True, **kw)
        out = ModelOutput(logits.cuda(), {"ctc_loss": 1.0}, loss=torch.tensor(1.0, device="cuda"),
                          logit_lens=lens.cuda())
        ev.track_batch(out, sample)
        return ev, out
    ev, out = run(lm_decode_test_predictions=True, lm_decode_arpa_path=TINY, lm_decode_unk_score_offset=UNK)
    ev0, out0 = run()
    lm = DeviceNgramLM.from_arpa(TINY, VOCAB, alpha=ALPHA, beta=BETA, device="cuda")
    t, n, _, _ = Fn.ctc_prefix_beam_lm(logits.cuda(), lens.cuda(), lm, beam=32, unk_score_offset=UNK,
                                       score_boundary=True)
    t, n = t.cpu().numpy(), n.cpu().numpy()
    pred = [cut_after_eos_token(tok.decode(list(t[b, :n[b]]), group_tokens=False)) for b in range(B)]
    labels = tok.batch_decode(target.numpy(), group_tokens=False)
    assert out.metrics["word_error_rate_lm_decode"] == word_error_rate(pred, labels)
    assert out.metrics["char_error_rate_lm_decode"] == char_error_rate(pred, labels)
    decoded = ev.evaluate().decoded[-1]
    assert decoded.predictions_lm_decoded == pred
    assert ev.evaluate().to_dict()["history"][0]["batch"]["predictions_lm_decoded"] == pred
    for k in ("word_error_rate", "char_error_rate", "ctc_loss"):
        assert out.metrics[k] == out0.metrics[k]
    assert "word_error_rate_lm_decode" not in out0.metrics
    assert decoded.predictions == ev0.evaluate().decoded[-1].predictions
    assert "predictions_lm_decoded" not in ev0.evaluate().to_dict()["history"][0]["batch"]
