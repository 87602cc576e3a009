"""Scope row 8f-1 on CPU: the BPE tokenizer against token ids produced by the reference's tokenizer, and the
oracle's CLIP text tower against the reference's CLIPTextEmbedding output (both committed as goldens)."""
import json
import os

import pytest
import torch

import diffsound_oracle as O
from conftest import GOLDEN, golden

NO_GRAD = True          # tests/conftest.py: every test of this module runs under torch.no_grad()
# the part of CLIP's merge table that the words of these tests exercise, with the original ranks and token ids
# (oracle/make_golden.py tokenizer_crosscheck(); the same format as the package's data/bpe_closed_vocab.json)
_TEST_BPE = os.path.join(GOLDEN, "bpe_test_vocab.json")


def _bpe_path():
    return _TEST_BPE


def clip_sd():
    from text_to_sound_synthesis_amd.synth import synth_state_dict
    with open(os.path.join(GOLDEN, "state_dict_keys_clip.json")) as f:
        return synth_state_dict(json.load(f))


def test_tokenizer_matches_reference_ids():
    from text_to_sound_synthesis_amd.tokenizer import Tokenize
    caps = json.load(open(os.path.join(GOLDEN, "captions.json")))
    g = golden("text_stage")
    t = Tokenize(context_length=77, add_start_and_end=True, with_mask=True, pad_value=0,
                 tokenizer_config={"params": {"end_idx": 49152}}, bpe_path=_bpe_path())
    out = t.get_tokens(caps)
    assert torch.equal(out["token"], g["tokens"])
    assert torch.equal(out["mask"], g["mask"])
    assert out["token"][-1, 0] == 49406 and out["token"][-1, -1] == 49407      # truncated caption keeps EOT
    assert (out["token"][0] == 49407).sum() == 1


def test_tokenizer_fails_loudly_without_vocab(monkeypatch, tmp_path):
    from text_to_sound_synthesis_amd import tokenizer as T
    monkeypatch.delenv("DIFFSOUND_BPE_PATH", raising=False)
    with pytest.raises(FileNotFoundError):
        T.Tokenize(context_length=77, bpe_path=str(tmp_path / "missing.gz")).get_tokens(["a dog"])


def test_oracle_clip_text_vs_reference():
    g = golden("text_stage")
    out = O.clip_text_embed(clip_sd(), g["tokens"])
    ref = g["cond_emb"]                        # the reference's CLIPTextEmbedding on all 8 captions
    assert out.shape == ref.shape == (8, 77, 512)
    assert (out.norm(dim=-1) - 1).abs().max() < 2e-3
    assert (out - ref).abs().max() < 1e-3      # same fp16 algorithm, same box: only op-fusion noise


def test_clip_state_dict_contract():
    from text_to_sound_synthesis_amd.config import build_model, default_config
    m = build_model(default_config(n_layer=1, with_clip=True))
    want = json.load(open(os.path.join(GOLDEN, "state_dict_keys_clip.json")))
    sd = {k: list(v.shape) for k, v in m.state_dict().items() if ".condition_emb." in k}
    assert sd == want


def random_captions():
    """2 000 random captions: words, digits, punctuation, apostrophes, HTML entities, odd spacing, upper case, a few
    non-ASCII letters, over-long captions (oracle/make_golden.py tokenizer_crosscheck() ran the reference on them)."""
    import random
    rng = random.Random(20260925)
    words = ["dog", "barks", "rain", "thunder", "engine", "a", "the", "while", "birds", "chirping", "loudly", "car",
             "passes", "by", "woman", "speaks", "and", "then", "laughs", "keyboard", "typing", "whoosh", "sizzling",
             "o'clock", "it's", "don't", "rock'n'roll", "3", "42", "1990s", "2x", "café", "naïve", "über", "&amp;",
             "&lt;b&gt;", "...", "!!", "?", ",", ";", ":", "-", "--", "(", ")", "\"quoted\"", "U.S.A.", "e-mail",
             "AC/DC", "100%", "#1", "@home", "under_score", "x" * 30, "Supercalifragilistic"]
    caps = []
    for _ in range(2000):
        n = rng.choice((1, 2, 5, 9, 15, 40, 120))
        toks = [rng.choice(words) for _ in range(n)]
        toks = [w.upper() if rng.random() < 0.1 else w.capitalize() if rng.random() < 0.1 else w for w in toks]
        sep = rng.choice((" ", " ", "  ", "\t", " \n "))
        caps.append(("  " if rng.random() < 0.2 else "") + sep.join(toks) + (" " if rng.random() < 0.2 else ""))
    return caps


def test_tokenizer_matches_live_reference_on_random_captions():
    """The 2 000 random captions of random_captions() through this package's tokenizer: ids and masks identical to what
    the reference's own SimpleTokenizer / clip.tokenize call path (tokenize.py:59-69) gave for them
    (tests/golden/tokenizer_random_captions.npz)."""
    import hashlib
    import numpy as np
    from text_to_sound_synthesis_amd.tokenizer import Tokenize
    caps = random_captions()
    with np.load(os.path.join(GOLDEN, "tokenizer_random_captions.npz")) as z:
        assert hashlib.sha256("\n".join(caps).encode()).hexdigest() == str(z["captions_sha256"])
        ref = {"token": torch.from_numpy(z["tokens"]).long(), "mask": torch.from_numpy(z["mask"])}
    kw = dict(context_length=77, add_start_and_end=True, with_mask=True, pad_value=0)
    mine = Tokenize(tokenizer_config={"params": {"end_idx": 49152}}, bpe_path=_bpe_path(), **kw)
    for i in range(0, len(caps), 250):
        a, b = ref["token"][i:i + 250], mine.get_tokens(caps[i:i + 250])
        assert torch.equal(a, b["token"]), [c for c, x, y in zip(caps[i:i + 250], a, b["token"]) if not torch.equal(x, y)][:3]
        assert torch.equal(ref["mask"][i:i + 250], b["mask"])


def test_closed_vocabulary_merge_table_matches_goldens_and_refuses_other_words():
    """data/bpe_closed_vocab.json (package data; what bench.py tokenises with on the GPU box): ids equal the reference's for
    captions over its word list (oracle/make_golden.py checked 3000 of them against the reference's tokenizer when the
    file was written; here: the committed golden captions that stay inside the word list), and a word outside the list
    raises instead of producing wrong ids."""
    import os
    import pytest
    from conftest import GOLDEN
    from text_to_sound_synthesis_amd import synth, tokenizer as tz
    closed = tz.SimpleTokenizer(bpe_path=tz.CLOSED_VOCAB_PATH)
    caps = synth.synth_captions(64, seed=7)
    tok = tz.tokenize(caps, context_length=77, add_start_and_end=True, tokenizer=closed)["token"]
    assert tok.shape == (64, 77) and (tok[:, 0] == 49406).all()
    for i, c in enumerate(caps):
        n = len(c.split())
        assert tok[i, 1 + n:].max() == 49407 and (tok[i, 1:1 + n] < 49406).all()     # >= one token per word, then EOT
    g = golden("text_stage")
    import json
    with open(os.path.join(GOLDEN, "captions.json")) as f:
        gold_caps = json.load(f)
    inside = [i for i, c in enumerate(gold_caps) if set(c.split()) <= closed.closed_words]
    assert len(inside) >= 6                                  # the six synthetic golden captions
    got = tz.tokenize([gold_caps[i] for i in inside], context_length=77, add_start_and_end=True, tokenizer=closed)["token"]
    assert torch.equal(got, g["tokens"][inside])
    with pytest.raises(KeyError):
        closed.encode("a saxophone plays")
