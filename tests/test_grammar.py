"""The grammar compiler (engines/grammar.py): regex subset -> minimised,
trimmed byte DFA -> per-state token tables.

Oracles are independent of the compiler: Python's `re` for acceptance (a
bytes pattern for ASCII patterns, the str pattern under re.ASCII for the
UTF-8 ones), a byte-by-byte walk for `next`, a BFS written here for `dist`,
json.loads for the verdict grammar."""

import json
import random
import re
from collections import deque

import numpy as np
import pytest

from sentio_amd.engines.bpe import get_tokenizer
from sentio_amd.engines.grammar import (MAX_STATES, VERDICT_GRAMMAR, Grammar,
                                        json_object_regex)
from sentio_amd.engines.tokenizer import BOS_ID, EOS_ID, PAD_ID

ASCII_PATTERNS = [
    r"abc",
    r"a|b|cd",
    r"a*",
    r"a+b*",
    r"(ab)?c",
    r"a?b?c?",
    r"(a|b)*abb",
    r"a{3}",
    r"a{2,4}",
    r"(ab){0,2}c",
    r"a{2,}b",
    r"x{,2}y",
    r"[abc]+",
    r"[a-f0-9]{1,4}",
    r"[^abc]x",
    r"[^a-y]+",
    r".a.",
    r".?end|x.*",
    r"\d+\.\d*",
    r"\w+@\w+",
    r"\s*-?\d{1,3}\s*",
    r"[\d\-+]+",
    r"\D\W\S",
    r"a\.b\*c\\d",
    r"\x41\x2a[\x30-\x39]",
    r"\{\"k\": ?(true|false)\}",
    r"(?:ab|cd)+e",
    r"((a|b)(c|d))*",
    r"[]a]+[a^]",
    r"a{,}b{x}",
    r"(|a)b",
    r"\t\n\r[\t ]*",
]

UTF8_PATTERNS = [
    r"é+",
    r"[^a]x",
    r".{2}",
    r"[α-ω]+!",
    r"\W\w",
    r"(日本|語)*",
    r"[^\x00-\x7f]+",
    r"[a😀-😏]{1,2}",
]

UNSUPPORTED = [
    r"a*?", r"a+?", r"a??", r"a{1,2}?", r"a*+", r"(?=a)b", r"(?!a)b",
    r"(?<=a)b", r"(a)\1", r"^a", r"a$", r"(?i)a", r"(?P<n>a)", r"\bword",
    r"\Aa", r"a\Z", r"a**", r"*a", r"(a", r"a)", r"[a", r"[b-a]", r"a{3,2}",
    r"\x4", r"\q", r"[[:alpha:]]", r"\xff", r"[\s-a]", r"[\d-a]", r"[a-\d]",
]


def dfa_random_walk(g: Grammar, rng: random.Random, max_len: int = 24,
                    alphabet: bytes | None = None):
    """A byte string from a random walk of the automaton (over `alphabet`
    when given) that stops at an accepting state with some probability."""
    s, out = 0, bytearray()
    for _ in range(max_len):
        if g.accepting[s] and rng.random() < 0.3:
            break
        moves = np.flatnonzero(g.trans[s] >= 0).tolist()
        if alphabet is not None:
            moves = [b for b in moves if b in alphabet]
        if not moves:
            break
        b = int(rng.choice(moves))
        out.append(b)
        s = int(g.trans[s, b])
    return bytes(out)


def mutate(data: bytes, alphabet: bytes, rng: random.Random) -> bytes:
    data = bytearray(data)
    for _ in range(rng.randint(1, 2)):
        op = rng.randint(0, 2)
        pos = rng.randint(0, len(data))
        if op == 0 or not data:
            data.insert(pos, rng.choice(alphabet))
        elif op == 1:
            del data[min(pos, len(data) - 1)]
        else:
            data[min(pos, len(data) - 1)] = rng.choice(alphabet)
    return bytes(data)


@pytest.mark.parametrize("pattern", ASCII_PATTERNS)
def test_dfa_equals_re_fullmatch_on_bytes(pattern):
    g = Grammar.from_regex(pattern)
    rx = re.compile(pattern.encode("ascii"))
    rng = random.Random(sum(map(ord, pattern)))
    # the pattern's alphabet is ASCII: beyond it `.` and negated classes
    # match whole UTF-8 scalars, which the next test checks
    alphabet = bytes(range(0x20, 0x7F)) + b"\t\n\r\x00"
    accepted = 0
    for i in range(300):
        walk = dfa_random_walk(g, rng, alphabet=alphabet)
        data = walk if i % 2 == 0 else mutate(walk, alphabet, rng)
        want = rx.fullmatch(data) is not None
        assert g.matches(data) == want, (pattern, data)
        accepted += want
    assert accepted > 0


@pytest.mark.parametrize("pattern", UTF8_PATTERNS)
def test_dfa_equals_re_ascii_on_utf8(pattern):
    """Beyond ASCII the automaton runs on UTF-8 and means what the str
    pattern means under re.ASCII: `.`, negated classes and \\W match one
    whole scalar."""
    g = Grammar.from_regex(pattern)
    rx = re.compile(pattern, re.ASCII)
    rng = random.Random(sum(map(ord, pattern)))
    pool = [c for c in pattern if ord(c) > 0x7F] + list("aéx!日語ω😀z\n")
    accepted = 0
    for i in range(300):
        # random walks give valid UTF-8 by construction; check and decode
        walk = dfa_random_walk(g, rng, 16)
        try:
            text = walk.decode("utf-8")
        except UnicodeDecodeError:
            # a walk cut off inside a scalar: not accepted, and no str to ask
            assert not g.matches(walk), (pattern, walk)
            continue
        if i % 2:
            chars = list(text)
            pos = rng.randint(0, len(chars))
            if chars and rng.random() < 0.4:
                del chars[min(pos, len(chars) - 1)]
            else:
                chars.insert(pos, rng.choice(pool))
            text = "".join(chars)
        want = rx.fullmatch(text) is not None
        assert g.matches(text.encode("utf-8")) == want, (pattern, text)
        accepted += want
    assert accepted > 0
    # never a lone continuation byte or a surrogate encoding
    for bad in (b"\x80", b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"):
        assert not Grammar.from_regex(r".+").matches(bad)


@pytest.mark.parametrize("pattern", UNSUPPORTED)
def test_unsupported_syntax_raises(pattern):
    with pytest.raises(ValueError):
        Grammar.from_regex(pattern)


def test_dfa_is_trimmed_and_minimal():
    g = Grammar.from_regex(r"(a|b)*abb")
    assert g.n_states == 4                      # the textbook minimal DFA
    for pattern in ASCII_PATTERNS[:12]:
        g = Grammar.from_regex(pattern)
        # every state reaches acceptance (BFS backwards)
        n = g.n_states
        ok = set(np.flatnonzero(g.accepting).tolist())
        grew = True
        while grew:
            grew = False
            for s in range(n):
                if s not in ok and any(int(t) in ok for t in g.trans[s]
                                       if t >= 0):
                    ok.add(s)
                    grew = True
        assert len(ok) == n, pattern
    with pytest.raises(ValueError):
        Grammar.from_regex(r"[ab]{120}", max_states=64)
    assert Grammar.from_regex(r"[ab]{120}", max_states=128).n_states == 121
    assert MAX_STATES == 32766


# ---------------------------------------------------------------- tables

@pytest.fixture(scope="module")
def tok():
    return get_tokenizer()


@pytest.fixture(scope="module", params=[r"(yes|no), [a-c]{2,5}!",
                                        r"\d+\.\d* ?(the|of|and)+",
                                        "verdict"])
def grammar_tables(request, tok):
    g = VERDICT_GRAMMAR if request.param == "verdict" \
        else Grammar.from_regex(request.param)
    return g, g.token_tables(tok)


def test_token_tables_shapes_and_specials(grammar_tables, tok):
    g, tb = grammar_tables
    nxt, mask, dist, start = tb.next, tb.mask, tb.dist, tb.start
    Vt, N = tok.vocab_size, g.n_states + 1
    done = N - 1
    assert nxt.dtype == np.int16 and nxt.shape == (N, Vt)
    assert mask.dtype == np.int32 and mask.shape == (N, (Vt + 31) // 32)
    assert dist.dtype == np.int16 and dist.shape == (N,)
    assert start == 0
    assert (nxt[:, [PAD_ID, BOS_ID]] == -1).all()
    empty = [t for t in range(Vt) if not tok.token_bytes[t] and t != EOS_ID]
    assert (nxt[:, empty] == -1).all()
    eos = nxt[:, EOS_ID]
    acc = np.concatenate([g.accepting, [True]])
    assert (eos[acc] == done).all() and (eos[~acc] == -1).all()
    assert (nxt[done, np.arange(Vt) != EOS_ID] == -1).all()
    # mask bits == (next >= 0), padding bits zero
    bits = ((mask.view(np.uint32)[:, :, None] >> np.arange(32, dtype=np.uint32))
            & 1).reshape(N, -1).astype(bool)
    assert (bits[:, :Vt] == (nxt >= 0)).all()
    assert not bits[:, Vt:].any()
    # every live state has an allowed token
    assert (nxt >= 0).any(axis=1).all()


def test_next_equals_a_byte_walk(grammar_tables, tok):
    g, tb = grammar_tables
    rng = random.Random(7)
    N, Vt = tb.next.shape
    for _ in range(3000):
        s, t = rng.randrange(N - 1), rng.randrange(3, Vt)
        want = g.walk(s, tok.token_bytes[t])
        assert int(tb.next[s, t]) == want, (s, t, tok.token_bytes[t])


def test_dist_equals_an_independent_bfs(grammar_tables):
    g, tb = grammar_tables
    nxt = tb.next
    N = nxt.shape[0]
    rev = [set() for _ in range(N)]
    for s in range(N):
        for t in set(nxt[s][nxt[s] >= 0].tolist()):
            rev[t].add(s)
    want = [None] * N
    q = deque()
    for s in range(N):
        if s == N - 1 or g.accepting[s]:
            want[s] = 0
            q.append(s)
    while q:
        t = q.popleft()
        for s in rev[t]:
            if want[s] is None:
                want[s] = want[t] + 1
                q.append(s)
    assert tb.dist.tolist() == want


def test_verdict_grammar_strings_parse(tok):
    from sentio_amd.pipeline.verifier import AnswerVerifier, extract_json_dict

    g = VERDICT_GRAMMAR
    rng = random.Random(11)
    seen_optional = 0
    for i in range(60):
        # token-level random walk to acceptance under a budget, by the
        # sampling rule: only tokens that can still finish in time
        tb = g.token_tables(tok)
        s, left, ids = 0, 60, []
        while True:
            allowed = [t for t in np.flatnonzero(tb.next[s] >= 0).tolist()
                       if tb.dist[tb.next[s, t]] <= left - 1]
            t = rng.choice(allowed)
            if t == EOS_ID:
                break
            ids.append(t)
            s, left = int(tb.next[s, t]), left - 1
            if left == 0:
                break
        text = tok.decode(ids)
        assert g.matches(text), text
        data = json.loads(text)
        assert list(data)[:3] == ["verdict", "citations_ok", "notes"]
        assert data["verdict"] in ("pass", "warn", "fail")
        assert isinstance(data["citations_ok"], bool)
        assert len(data["notes"]) <= 4
        assert all(isinstance(n, str) for n in data["notes"])
        seen_optional += "revised_answer" in data
        out = AnswerVerifier._normalize(extract_json_dict(text))
        assert out["notes"] != ["invalid_json"]
        assert out["verdict"] == data["verdict"]
    assert seen_optional > 0
    assert not g.matches('{"verdict": "maybe", "citations_ok":true, '
                         '"notes": []}')
    assert not g.matches('{"citations_ok":true, "verdict": "pass", '
                         '"notes": []}')           # fixed key order
    assert not g.matches('{"verdict": "pass", "citations_ok":true, "notes": '
                         '["a", "b", "c", "d", "e"]}')


def test_json_object_fields():
    g = Grammar.json_object([
        {"name": "n", "type": "integer"},
        {"name": "s", "type": "string"},
        {"name": "tags", "type": "array", "max_items": 2, "optional": True},
    ])
    for text, want in [('{"n": 12, "s": "a\\"b"}', True),
                       ('{"n":-7,"s":"","tags":["x","y"]}', True),
                       ('{"n": 0, "s": "é\\u00e9", "tags": []}', True),
                       ('{"n": 01, "s": ""}', False),
                       ('{"n": 1, "s": "a\nb"}', False),
                       ('{"n": 1,  "s": ""}', False),      # two spaces
                       ('{"n": 1, "s": "", "tags": ["a","b","c"]}', False)]:
        assert g.matches(text) == want, text
        if want:
            json.loads(text)
    assert Grammar.json_object([]).matches("{}")
    with pytest.raises(ValueError):
        json_object_regex([{"name": "a", "type": "string", "optional": True},
                           {"name": "b", "type": "string"}])
    with pytest.raises(ValueError):
        json_object_regex([{"name": "a", "type": "float"}])
