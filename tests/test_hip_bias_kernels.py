"""The phrase automaton on the device alone (csrc/bias.hip) through include/masr_test.h: masr_test_bias_step -- the __device__
step the sweep calls -- against tests/bias_ref.py on random states and tokens, the table's probing, and what masr_bias_create refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import masr_amd  # noqa: E402,F401
import bias_ref  # noqa: E402
from masr_amd._cabi import MasrError, lib  # noqa: E402
from masr_amd.bias import ContextBias  # noqa: E402

DEV = "cuda:0"

LISTS = {
    # a phrase that is a prefix of another, a single-token phrase, shared prefixes
    "prefix_and_single": (12, [[3, 4], [3, 4, 5, 6], [7], [3, 8], [9, 9, 2], [2, 3, 4, 1]]),
    # repeated tokens: the restart at the root with the token that broke the match
    "repeats": (5, [[1, 1, 2], [2, 2], [3, 1, 1, 3], [1, 2, 3]]),
    "wide": (4096, None),                                       # bias_ref.toy_phrases(4096, 3000, 3, 6)
}


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def phrases_of(name):
    Cn, ph = LISTS[name]
    return Cn, ph if ph is not None else bias_ref.toy_phrases(Cn, 3000, 3, 6)


@pytest.mark.parametrize("name", list(LISTS))
def test_step_matches_the_restatement(name):
    Cn, phrases = phrases_of(name)
    trie = bias_ref.build(phrases)
    dev = ContextBias(Cn, phrases)
    l = lib()
    assert dev.nodes == trie["nodes"] and dev.bytes > 0 and dev.phrases == len(phrases)
    assert l.masr_test_bias_max_probe(dev.h) == bias_ref.table_max_probe(trie)
    if name == "wide":
        assert len(phrases) == 3000 and l.masr_test_bias_max_probe(dev.h) >= 2      # linear probing is exercised
    rng = np.random.default_rng(7)
    n = 20000
    nodes = rng.integers(0, trie["nodes"], size=n).astype(np.int32)
    # a state the search can be in: at least the running match's tokens are credited
    cnt = (np.asarray(trie["depth"], np.int32)[nodes] + rng.integers(0, 5, size=n)).astype(np.int32)
    # half the tokens continue the state's match where it has a child, the rest are any class (blank and eos included: they have no child)
    kids = {}
    for (u, c), v in trie["child"].items():
        kids.setdefault(u, []).append(c)
    tok = rng.integers(0, Cn, size=n).astype(np.int32)
    for i in range(0, n, 2):
        if int(nodes[i]) in kids:
            tok[i] = kids[int(nodes[i])][int(rng.integers(len(kids[int(nodes[i])])))]
    want = [bias_ref.step(trie, (int(u), int(c)), int(t)) for u, c, t in zip(nodes, cnt, tok)]
    assert sum(w[0] != 0 for w in want) > n // 8 and sum(bias_ref.revoked_by(trie, (int(u), 0), int(t)) > 0 for u, t in zip(nodes, tok)) > n // 8
    d = [torch.from_numpy(a).to(DEV) for a in (nodes, cnt, tok)]
    out = [torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=DEV) for _ in range(2)]
    assert l.masr_test_bias_step(dev.h, *map(p, d), n, *map(p, out), None) == 0, l.masr_last_error()
    got_u, got_n = (t.cpu().numpy() for t in out)
    assert np.array_equal(got_u, np.asarray([w[0] for w in want], np.int32))
    assert np.array_equal(got_n, np.asarray([w[1] for w in want], np.int32))
    # whole sequences, token by token through the device step, end where the restatement's do
    seqs = [[int(c) for c in rng.integers(1, min(Cn - 1, 9), size=12)] for _ in range(64)] + [list(ph) + list(ph) for ph in phrases[:64]]
    L = max(len(s) for s in seqs)
    su, sn = torch.zeros(len(seqs), dtype=torch.int32, device=DEV), torch.zeros(len(seqs), dtype=torch.int32, device=DEV)
    for i in range(L):
        t = torch.tensor([s[i] if i < len(s) else 0 for s in seqs], dtype=torch.int32, device=DEV)     # (class 0 past the end: back to the root)
        nu, nn = torch.empty_like(su), torch.empty_like(sn)
        assert l.masr_test_bias_step(dev.h, p(su), p(sn), p(t), len(seqs), p(nu), p(nn), None) == 0
        su, sn = nu, nn
    want = [bias_ref.state_of(trie, s + [0] * (L - len(s))) for s in seqs]
    assert su.cpu().tolist() == [w[0] for w in want] and sn.cpu().tolist() == [w[1] for w in want]
    dev.close()
    assert dev.h is None


def test_step_entry_refusals():
    l = lib()
    dev = ContextBias(12, [[3, 4]])
    a = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert l.masr_test_bias_step(None, p(a), p(a), p(a), 4, p(a), p(a), None) == -1
    assert l.masr_test_bias_step(dev.h, p(a), p(a), p(a), 0, p(a), p(a), None) == -1
    assert l.masr_test_bias_max_probe(None) == -1 and l.masr_bias_bytes(None) == -1
    # a node outside the trie is answered with (-1, -1), not looked up
    nodes = torch.tensor([0, 3, -1, 99], dtype=torch.int32, device=DEV)
    out = [torch.full((4,), 77, dtype=torch.int32, device=DEV) for _ in range(2)]
    assert l.masr_test_bias_step(dev.h, p(nodes), p(a), p(a), 4, *map(p, out), None) == 0
    assert out[0].cpu().tolist() == [0, -1, -1, -1] and out[1].cpu().tolist() == [0, -1, -1, -1]


def test_builder_refusals():
    l = lib()

    def refused(Cn, phrases):
        with pytest.raises(MasrError) as e:
            ContextBias(Cn, phrases)
        return str(e.value)
    assert "the number of classes must be in [3, 65535]" in refused(2, [[1]])
    assert "the number of classes must be in [3, 65535]" in refused(65536, [[1]])
    assert "the number of phrases must be in [1, 65536]" in refused(12, [])
    assert "the number of phrases must be in [1, 65536]" in refused(12, [[1 + i % 10, 1 + i // 10 % 10, 1 + i // 100 % 10, 1 + i // 1000 % 10, 1 + i // 10000]
                                                                         for i in range(65537)])
    assert "a phrase must hold 1 to 64 tokens" in refused(12, [[3, 4], []])
    assert "a phrase must hold 1 to 64 tokens" in refused(12, [[3] * 65])
    assert "a phrase holds a token outside [1, C - 2]" in refused(12, [[3, 0]])
    assert "a phrase holds a token outside [1, C - 2]" in refused(12, [[3, 11]])
    assert "a phrase holds a token outside [1, C - 2]" in refused(12, [[-1]])
    assert "duplicate phrase" in refused(12, [[3, 4], [5], [3, 4]])
    # 17000 phrases of 64 tokens that share nothing: 1 088 000 distinct prefixes
    many = [[1 + i] + [1 + (7 * i + j) % 16000 for j in range(1, 64)] for i in range(17000)]
    assert "more than 2^20 distinct prefixes" in refused(20000, many)
    tok = (C.c_int32 * 2)(3, 4)
    off = (C.c_int64 * 2)(0, 2)
    assert not l.masr_bias_create(12, 1, None, off) and b"null pointer" in l.masr_last_error()
    assert not l.masr_bias_create(12, 1, tok, None) and b"null pointer" in l.masr_last_error()
    # the limits themselves are accepted
    ok = ContextBias(12, [[3] * 64, [4]])
    assert ok.nodes == 66
    ok.close()
