"""The phrase automaton of contextual biasing (include/masr.h) on Python dicts, for tests/ctc_bias_beam_ref.py and the tests of
csrc/bias.hip.  A plain helper module like lm_ref.py.

build(phrases) -> the trie: nodes are numbered in creation order while the phrases are inserted one after the other, token by token (the
order masr_bias_create numbers them in, so node ids can be compared), the root is node 0.
  child    {(node, token): node}
  depth    [nodes]
  revoke   [nodes]: depth(u) - e(u), e(u) = the length of the longest phrase that is a prefix of, or equal to, u's string
A state is (node, credited tokens).  There are no failure links: a broken match restarts at the root with the current token."""
import numpy as np

MAX_PHRASE = 64


def build(phrases):
    child, parent, depth, terminal = {}, [-1], [0], [False]
    for p in phrases:
        assert 1 <= len(p) <= MAX_PHRASE
        u = 0
        for c in p:
            v = child.get((u, int(c)))
            if v is None:
                v = child[(u, int(c))] = len(parent)
                parent.append(u)
                depth.append(depth[u] + 1)
                terminal.append(False)
            u = v
        assert not terminal[u], "duplicate phrase"
        terminal[u] = True
    earned = [0] * len(parent)
    for u in range(1, len(parent)):
        earned[u] = depth[u] if terminal[u] else earned[parent[u]]
    return {"child": child, "depth": depth, "revoke": [d - e for d, e in zip(depth, earned)], "nodes": len(parent), "phrases": len(phrases)}


ROOT = (0, 0)


def step(trie, state, c, mutate=None):
    """the state behind token c; mutate: "no_revoke" keeps the tokens of a broken match, "no_retry_from_root" drops the token that broke it"""
    u, n = state
    v = trie["child"].get((u, c))
    if v is not None:
        return (v, n + 1)
    if mutate != "no_revoke":
        n -= trie["revoke"][u]
    if mutate == "no_retry_from_root":
        return (0, n)
    v = trie["child"].get((0, c))
    if v is not None:
        return (v, n + 1)
    return (0, n)


def revoked_by(trie, state, c):
    """the tokens step() takes back on this token (0: the match goes on, or nothing was pending)"""
    u, _ = state
    return 0 if (u, c) in trie["child"] else trie["revoke"][u]


def n_final(trie, state, mutate=None):
    u, n = state
    return n if mutate == "no_final_revoke" else n - trie["revoke"][u]


def state_of(trie, h, mutate=None):
    s = ROOT
    for c in h:
        s = step(trie, s, int(c), mutate)
    return s


def count(trie, h, mutate=None):
    """n_final of the token sequence h"""
    return n_final(trie, state_of(trie, h, mutate), mutate)


def toy_phrases(C, P, seed, maxlen=6, minlen=1):
    """P distinct random phrases over the tokens 1 .. C - 2, lengths in [minlen, maxlen]; about a third are a prefix of another phrase plus
    more tokens, so shared prefixes and phrases inside phrases occur"""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < P:
        n = int(rng.integers(minlen, maxlen + 1))
        if out and rng.random() < 0.33:
            base = out[int(rng.integers(len(out)))]
            p = tuple(base[:maxlen - 1]) + tuple(int(t) for t in rng.integers(1, C - 1, size=1))
        else:
            p = tuple(int(t) for t in rng.integers(1, C - 1, size=n))
        if p not in seen:
            seen.add(p)
            out.append(list(p))
    return out


def flatten(phrases):
    """-> (tokens int32 [sum], off int64 [P + 1]) as masr_bias_create takes them"""
    off = np.zeros(len(phrases) + 1, np.int64)
    off[1:] = np.cumsum([len(p) for p in phrases])
    return np.asarray([t for p in phrases for t in p], np.int32), off


def table_max_probe(trie):
    """the longest probe chain (slots examined) an insertion walks when masr_bias_create builds this trie's table: edges inserted in child-node
    order, key = (node + 1) << 16 | (token + 1), capacity a power of two >= 2 x the edges and >= 16, the n-gram tables' multiplicative hash"""
    edges = sorted((v, u, c) for (u, c), v in trie["child"].items())
    cap, bits = 16, 4
    while cap < 2 * len(edges):
        cap, bits = cap * 2, bits + 1
    used, worst = set(), 0
    for _, u, c in edges:
        key = ((u + 1) << 16) | (c + 1)
        at = ((key * 0x9E3779B97F4A7C15) & (2 ** 64 - 1)) >> (64 - bits)
        probes = 1
        while at & (cap - 1) in used:
            at, probes = at + 1, probes + 1
        used.add(at & (cap - 1))
        worst = max(worst, probes)
    return worst
