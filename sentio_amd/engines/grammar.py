"""Grammar-constrained decoding: regex -> byte DFA -> per-state token tables.

`Grammar.from_regex` compiles a regex subset to a minimised, trimmed DFA
over BYTES (every state can reach an accepting state).  The subset:
literals, `.`, escapes (`\\n \\t \\r \\f \\v \\0 \\xHH`, `\\d \\w \\s` and their
negations, escaped punctuation), character classes with ranges and negation,
groups `( )` / `(?: )`, `|`, `*`, `+`, `?`, `{m}`, `{m,n}`, `{m,}`, `{,n}`.
Matching is anchored at both ends (re.fullmatch).  Everything else raises
ValueError: anchors, backreferences, lookaround, lazy or possessive
quantifiers, flags, named groups.

Semantics are Python `re`'s on a bytes pattern for ASCII input.  Beyond
ASCII the automaton works on UTF-8: a non-ASCII literal is its bytes, and
`.`, negated classes and `\\D \\W \\S` match ONE well-formed UTF-8 scalar
(Unicode Table 3-7 byte ranges, no surrogates), never a lone continuation
byte -- the str pattern under `re.ASCII`.  Constrained output therefore
always decodes.

`Grammar.token_tables(tokenizer)` lifts the DFA to the tokenizer's
vocabulary: `next[s, t]` walks token t's bytes from state s, `mask` is its
bitset, `dist[s]` the fewest tokens from s to acceptance.  The sampler
(ops.sample_constrained) masks by state, keeps a row inside its token budget
with `dist`, and advances the state on the device.
"""

from __future__ import annotations

import time
import weakref
from dataclasses import dataclass

import numpy as np

from sentio_amd.engines.tokenizer import BOS_ID, EOS_ID, PAD_ID

MAX_STATES = 32766          # int16 tables: states 0..32765 plus DONE
API_MAX_STATES = 2048       # cap for patterns that arrive through the API
API_COMPILE_SECONDS = 1.0   # wall-clock budget of one API pattern's compile
_MAX_NFA = 200_000


class _Budget:
    """What one compile may spend: NFA states, subset-construction work
    (edges scanned, a deterministic count) and, optionally, wall-clock
    seconds.  Both scale with the state limit, so a pattern that arrives
    through the API (API_MAX_STATES) is turned down after a fraction of a
    second, long before the limit on the RESULT could be checked."""

    def __init__(self, max_states: int, seconds: float | None):
        self.max_nfa = min(_MAX_NFA, 16 * max_states + 1024)
        self.max_work = 1500 * max_states + 1_000_000
        self.work = 0
        self.deadline = None if seconds is None \
            else time.perf_counter() + float(seconds)

    def spend(self, work: int = 0) -> None:
        self.work += work
        if self.work > self.max_work or (
                self.deadline is not None
                and time.perf_counter() > self.deadline):
            raise ValueError("pattern too large: compiling it exceeds the "
                             "work budget for this state limit")
_MAX_CP = 0x10FFFF
_SUR_LO, _SUR_HI = 0xD800, 0xDFFF

_DIGIT = [(0x30, 0x39)]
_WORD = [(0x30, 0x39), (0x41, 0x5A), (0x5F, 0x5F), (0x61, 0x7A)]
_SPACE = [(0x09, 0x0D), (0x20, 0x20)]
_SIMPLE_ESC = {"n": 0x0A, "t": 0x09, "r": 0x0D, "f": 0x0C, "v": 0x0B,
               "a": 0x07, "0": 0x00}
_SPECIAL = set("\\.[](){}|*+?^$")


# ---------------------------------------------------------------- ranges
def _norm(ranges):
    """Sorted, merged code point ranges without surrogates."""
    out = []
    for lo, hi in sorted(ranges):
        if out and lo <= out[-1][1] + 1:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    res = []
    for lo, hi in out:
        if lo < _SUR_LO and hi >= _SUR_LO:
            res.append((lo, _SUR_LO - 1))
            lo = _SUR_LO
        if lo >= _SUR_LO and lo <= _SUR_HI:
            lo = _SUR_HI + 1
        if lo <= hi:
            res.append((lo, hi))
    return res


def _negate(ranges):
    out, prev = [], 0
    for lo, hi in _norm(ranges):
        if lo > prev:
            out.append((prev, lo - 1))
        prev = hi + 1
    if prev <= _MAX_CP:
        out.append((prev, _MAX_CP))
    return _norm(out)


def _enc(cp: int) -> bytes:
    return chr(cp).encode("utf-8")


def _utf8_seqs(lo: int, hi: int, n: int):
    """Byte-range sequences matching the code points lo..hi, all of which
    encode to n bytes (the utf8-ranges split: cut until the leading bytes
    agree wherever the trailing ones are not full)."""
    if n == 1:
        return [[(lo, hi)]]
    for i in range(1, n):
        m = (1 << (6 * i)) - 1
        if (lo & ~m) != (hi & ~m):
            if lo & m:
                return (_utf8_seqs(lo, lo | m, n)
                        + _utf8_seqs((lo | m) + 1, hi, n))
            if (hi & m) != m:
                return (_utf8_seqs(lo, (hi & ~m) - 1, n)
                        + _utf8_seqs(hi & ~m, hi, n))
    return [list(zip(_enc(lo), _enc(hi)))]


def _class_seqs(ranges):
    """Code point ranges -> list of byte-range sequences (well-formed UTF-8)."""
    seqs = []
    for lo, hi in _norm(ranges):
        for n, (a, b) in enumerate(((0, 0x7F), (0x80, 0x7FF),
                                    (0x800, 0xFFFF), (0x10000, _MAX_CP)), 1):
            l, h = max(lo, a), min(hi, b)
            if l > h:
                continue
            # surrogates are already cut out by _norm
            seqs.extend(_utf8_seqs(l, h, n))
    return seqs


# ---------------------------------------------------------------- parser
# AST: ("cls", ranges) | ("cat", [nodes]) | ("alt", [nodes])
#      | ("rep", node, lo, hi|None) | ("eps",)
class _Parser:
    def __init__(self, pattern: str):
        if not isinstance(pattern, str):
            raise ValueError("pattern must be a str")
        self.p = pattern
        self.i = 0

    def err(self, msg: str):
        raise ValueError(f"unsupported regex at position {self.i}: {msg} "
                         f"(pattern {self.p!r})")

    def peek(self):
        return self.p[self.i] if self.i < len(self.p) else None

    def parse(self):
        node = self.alt()
        if self.i != len(self.p):
            self.err("unbalanced ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == "|":
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ("alt", branches)

    def cat(self):
        items = []
        while self.peek() is not None and self.peek() not in "|)":
            atom = self.atom()
            items.append(self.quant(atom))
        if not items:
            return ("eps",)
        return items[0] if len(items) == 1 else ("cat", items)

    def quant(self, atom):
        c = self.peek()
        lo = hi = None
        if c == "*":
            lo, hi = 0, None
            self.i += 1
        elif c == "+":
            lo, hi = 1, None
            self.i += 1
        elif c == "?":
            lo, hi = 0, 1
            self.i += 1
        elif c == "{":
            q = self.braces()
            if q is None:
                return atom          # a literal '{': the next atom
            lo, hi = q
        else:
            return atom
        if self.peek() in ("?", "+"):
            self.err("lazy and possessive quantifiers")
        if self.peek() == "*" or (self.peek() == "{"
                                  and self.braces(peek=True) is not None):
            self.err("multiple repeat")
        if hi is not None and hi < lo:
            self.err("min repeat greater than max repeat")
        return ("rep", atom, lo, hi)

    def braces(self, peek: bool = False):
        """`{m}`, `{m,n}`, `{m,}`, `{,n}` at self.i -> (lo, hi) and consume;
        None (nothing consumed) when the brace is a literal, as in `re`."""
        j = self.i + 1
        p = self.p
        if j < len(p) and p[j] == "}":
            return None
        k = j
        while k < len(p) and p[k].isdigit() and p[k].isascii():
            k += 1
        lo_s = p[j:k]
        if k < len(p) and p[k] == ",":
            k += 1
            j2 = k
            while k < len(p) and p[k].isdigit() and p[k].isascii():
                k += 1
            hi_s = p[j2:k]
            comma = True
        else:
            hi_s, comma = lo_s, False
        if k >= len(p) or p[k] != "}":
            return None
        lo = int(lo_s) if lo_s else 0
        hi = int(hi_s) if hi_s else None
        if not comma and not lo_s:
            return None
        if not peek:
            self.i = k + 1
        return lo, hi

    def atom(self):
        c = self.peek()
        if c == "(":
            self.i += 1
            if self.peek() == "?":
                if self.p[self.i:self.i + 2] == "?:":
                    self.i += 2
                else:
                    self.err("only plain and (?:...) groups: no lookaround, "
                             "flags or named groups")
            node = self.alt()
            if self.peek() != ")":
                self.err("missing ')'")
            self.i += 1
            return node
        if c == "[":
            return ("cls", self.cls())
        if c == ".":
            self.i += 1
            return ("cls", _negate([(0x0A, 0x0A)]))
        if c == "\\":
            return ("cls", self.escape(in_class=False)[1])
        if c in "*+?":
            self.err("nothing to repeat")
        if c == "{":
            if self.braces(peek=True) is not None:
                self.err("nothing to repeat")
        if c in "^$":
            self.err("anchors (matching is always anchored at both ends)")
        self.i += 1
        return ("cls", [(ord(c), ord(c))])

    def escape(self, in_class: bool):
        """At a backslash -> ("lit", [(c, c)]) or ("set", ranges)."""
        self.i += 1
        c = self.peek()
        if c is None:
            self.err("trailing backslash")
        self.i += 1
        if c in "dDwWsS":
            base = {"d": _DIGIT, "w": _WORD, "s": _SPACE}[c.lower()]
            return "set", (_norm(base) if c.islower() else _negate(base))
        if c == "x":
            h = self.p[self.i:self.i + 2]
            if len(h) != 2 or any(ch not in "0123456789abcdefABCDEF"
                                  for ch in h):
                self.err("\\x needs two hex digits")
            self.i += 2
            v = int(h, 16)
            if v > 0x7F:
                self.err("\\x escapes above 7f (write the character itself)")
            return "lit", [(v, v)]
        if c in _SIMPLE_ESC and not (c == "0" and (self.peek() or "x").isdigit()):
            return "lit", [(_SIMPLE_ESC[c], _SIMPLE_ESC[c])]
        if c == "b" and in_class:
            return "lit", [(0x08, 0x08)]
        if c.isdigit():
            self.err("backreferences and octal escapes")
        if c.isascii() and c.isalpha():
            self.err(f"escape \\{c}")
        return "lit", [(ord(c), ord(c))]

    def cls(self):
        self.i += 1                       # '['
        neg = False
        if self.peek() == "^":
            neg = True
            self.i += 1
        ranges = []
        first = True
        while True:
            c = self.peek()
            if c is None:
                self.err("unterminated character class")
            if c == "]" and not first:
                self.i += 1
                break
            first = False
            if c == "[" and self.p[self.i:self.i + 2] in ("[:", "[.", "[="):
                self.err("POSIX classes")
            if c == "\\":
                kind, val = self.escape(in_class=True)
            else:
                self.i += 1
                kind, val = "lit", [(ord(c), ord(c))]
            is_range = (self.peek() == "-" and self.i + 1 < len(self.p)
                        and self.p[self.i + 1] != "]")
            if is_range and kind == "set":
                self.err("bad character range")     # [\s-a], as in `re`
            if is_range:
                self.i += 1
                c2 = self.peek()
                if c2 == "\\":
                    kind2, val2 = self.escape(in_class=True)
                    if kind2 != "lit":
                        self.err("bad character range")
                else:
                    self.i += 1
                    val2 = [(ord(c2), ord(c2))]
                if val2[0][0] < val[0][0]:
                    self.err("bad character range")
                ranges.append((val[0][0], val2[0][0]))
            else:
                ranges.extend(val)
        ranges = _negate(ranges) if neg else _norm(ranges)
        return ranges


# ---------------------------------------------------------------- NFA
class _NFA:
    def __init__(self, budget: _Budget):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple[int, int, int]]] = []   # (lo, hi, dst)
        self.budget = budget

    def new(self) -> int:
        if len(self.eps) >= self.budget.max_nfa:
            raise ValueError("pattern too large: the automaton exceeds "
                             f"{self.budget.max_nfa} NFA states")
        if len(self.eps) % 1024 == 0:
            self.budget.spend()
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def build(self, node) -> tuple[int, int]:
        kind = node[0]
        if kind == "eps":
            s = self.new()
            return s, s
        if kind == "cls":
            s, e = self.new(), self.new()
            for seq in _class_seqs(node[1]):
                cur = s
                for j, (lo, hi) in enumerate(seq):
                    nxt = e if j == len(seq) - 1 else self.new()
                    self.edges[cur].append((lo, hi, nxt))
                    cur = nxt
            return s, e
        if kind == "cat":
            s, e = self.build(node[1][0])
            for sub in node[1][1:]:
                s2, e2 = self.build(sub)
                self.eps[e].append(s2)
                e = e2
            return s, e
        if kind == "alt":
            s, e = self.new(), self.new()
            for sub in node[1]:
                s2, e2 = self.build(sub)
                self.eps[s].append(s2)
                self.eps[e2].append(e)
            return s, e
        if kind == "rep":
            _, sub, lo, hi = node
            s = self.new()
            e = s
            for _ in range(lo):
                s2, e2 = self.build(sub)
                self.eps[e].append(s2)
                e = e2
            if hi is None:
                s2, e2 = self.build(sub)
                loop = self.new()
                self.eps[e].append(loop)
                self.eps[loop].append(s2)
                self.eps[e2].append(loop)
                e = loop
            else:
                end = self.new()
                for _ in range(hi - lo):
                    s2, e2 = self.build(sub)
                    self.eps[e].append(end)
                    self.eps[e].append(s2)
                    e = e2
                self.eps[e].append(end)
                e = end
            return s, e
        raise AssertionError(kind)


def _determinise(nfa: _NFA, start: int, accept: int, max_states: int):
    """Subset construction -> (trans int32 [n, 256] with -1, accepting bool)."""
    budget = nfa.budget
    closure_cache: dict[int, frozenset] = {}

    def closure(states):
        out = set()
        stack = list(states)
        while stack:
            s = stack.pop()
            if s in out:
                continue
            out.add(s)
            stack.extend(nfa.eps[s])
        return frozenset(out)

    # byte equivalence classes from every edge boundary
    cut = np.zeros(257, dtype=bool)
    cut[0] = True
    for es in nfa.edges:
        for lo, hi, _ in es:
            cut[lo] = True
            cut[hi + 1] = True
    reps = [b for b in range(256) if cut[b]]
    cls_of = np.cumsum(cut[:256]) - 1

    s0 = closure([start])
    ids = {s0: 0}
    order = [s0]
    rows = []
    i = 0
    while i < len(order):
        cur = order[i]
        i += 1
        row = [-1] * len(reps)
        edges = [e for s in cur for e in nfa.edges[s]]
        budget.spend(len(cur) + len(edges) * len(reps))
        if edges:
            for ci, b in enumerate(reps):
                dst = {d for lo, hi, d in edges if lo <= b <= hi}
                if not dst:
                    continue
                key = None
                if len(dst) == 1:
                    d = next(iter(dst))
                    key = closure_cache.get(d)
                    if key is None:
                        key = closure_cache[d] = closure(dst)
                else:
                    key = closure(dst)
                j = ids.get(key)
                if j is None:
                    j = ids[key] = len(order)
                    order.append(key)
                    if len(order) > 2 * max_states + 64:
                        raise ValueError(
                            f"pattern too large: more than {max_states} "
                            "automaton states")
                row[ci] = j
        rows.append(row)
    small = np.asarray(rows, dtype=np.int32).reshape(len(order), len(reps))
    trans = small[:, cls_of]
    accepting = np.fromiter((accept in st for st in order), dtype=bool,
                            count=len(order))
    return trans, accepting


def _trim_minimise(trans: np.ndarray, accepting: np.ndarray,
                   budget: _Budget):
    """Drop states that cannot reach acceptance, merge equivalent states
    (Moore refinement), renumber breadth-first from the start state."""
    n = trans.shape[0]
    # co-reachability
    src, col = np.nonzero(trans >= 0)
    edges = np.unique(src.astype(np.int64) * n + trans[src, col])
    e_src, e_dst = edges // n, edges % n
    live = accepting.copy()
    frontier = live.copy()
    while frontier.any():               # backwards, one frontier at a time
        hit = np.zeros(n, dtype=bool)
        hit[e_src[frontier[e_dst]]] = True
        frontier = hit & ~live
        live |= frontier
    if not live[0]:
        raise ValueError("the pattern matches nothing")
    trans = np.where((trans >= 0) & live[np.clip(trans, 0, n - 1)], trans, -1)
    keep = np.flatnonzero(live)
    remap = np.full(n + 1, -1, dtype=np.int64)
    remap[keep] = np.arange(keep.size)
    trans = remap[trans[keep]]            # -1 indexes the sentinel
    accepting = accepting[keep]
    n = keep.size
    # Moore: block of a state = (block, blocks of its successors), over the
    # distinct byte columns only (a refinement pass costs n x classes)
    full = trans
    trans = np.unique(trans, axis=1)
    block = accepting.astype(np.int64)
    nblocks = len(np.unique(block))
    # Two phases.  First the signature rows are compared through a 64-bit
    # multilinear hash with fixed odd multipliers (wrap-around arithmetic):
    # sorting n integers instead of n rows keeps a long chain, which needs
    # one pass per state, cheap.  A hash collision could only leave two
    # inequivalent states in one block, never split equivalent ones, so the
    # second phase goes on refining on the EXACT rows until nothing changes:
    # normally one confirming pass, and the result never rests on the hash.
    mult = (np.random.RandomState(2024).randint(
        1, 2 ** 62, size=trans.shape[1] + 1, dtype=np.int64) * 2 + 1)
    exact = False
    while True:
        budget.spend()
        ext = np.concatenate([block, [-1]])
        if exact:
            sig = np.concatenate([block[:, None], ext[trans]], axis=1)
            _, new = np.unique(sig, axis=0, return_inverse=True)
        else:
            with np.errstate(over="ignore"):
                sig = block * mult[0] + (ext[trans] * mult[1:]).sum(axis=1)
            _, new = np.unique(sig, return_inverse=True)
        new = new.reshape(-1)
        nb = int(new.max()) + 1
        block = new.astype(np.int64)
        if nb == nblocks:
            if exact:
                break
            exact = True
        nblocks = nb
    # one representative per block, BFS order from the start's block
    rep = np.full(nblocks, -1, dtype=np.int64)
    for s in range(n - 1, -1, -1):
        rep[block[s]] = s
    ext = np.concatenate([block, [-1]])
    btrans = ext[full[rep]]               # [nblocks, 256] over blocks
    order = [int(block[0])]
    seen = {order[0]}
    i = 0
    while i < len(order):
        for t in np.unique(btrans[order[i]]):
            t = int(t)
            if t >= 0 and t not in seen:
                seen.add(t)
                order.append(t)
        i += 1
    order = np.asarray(order, dtype=np.int64)
    pos = np.full(nblocks + 1, -1, dtype=np.int64)
    pos[order] = np.arange(order.size)
    out = pos[btrans[order]].astype(np.int32)
    acc = accepting[rep[order]]
    return out, acc


# ---------------------------------------------------------------- tables
@dataclass
class TokenTables:
    """Host tables of one grammar over one tokenizer (numpy).  N states:
    the DFA's plus DONE (index N - 1)."""

    next: np.ndarray          # int16 [N, Vt]
    mask: np.ndarray          # int32 [N, ceil(Vt / 32)]
    dist: np.ndarray          # int16 [N]
    start: int
    build_s: float = 0.0

    @property
    def n_states(self) -> int:
        return int(self.next.shape[0])

    @property
    def vocab(self) -> int:
        return int(self.next.shape[1])

    @property
    def done(self) -> int:
        return self.n_states - 1

    @property
    def nbytes(self) -> int:
        return int(self.next.nbytes + self.mask.nbytes + self.dist.nbytes)


def pack_mask(nxt: np.ndarray) -> np.ndarray:
    """int32 [N, ceil(Vt/32)] bitset of next >= 0; padding bits are 0."""
    N, Vt = nxt.shape
    W = (Vt + 31) // 32
    bits = np.zeros((N, W * 32), dtype=bool)
    bits[:, :Vt] = nxt >= 0
    packed = np.packbits(bits.reshape(N, W, 32), axis=2, bitorder="little")
    return np.ascontiguousarray(packed).view("<u4").reshape(N, W) \
        .astype(np.uint32).view(np.int32)


class Grammar:
    """A trimmed, minimised byte DFA.  trans int32 [n, 256] (-1: no move),
    accepting bool [n], start state 0."""

    def __init__(self, trans: np.ndarray, accepting: np.ndarray,
                 pattern: str = ""):
        self.trans = np.ascontiguousarray(trans, dtype=np.int32)
        self.accepting = np.ascontiguousarray(accepting, dtype=bool)
        self.pattern = pattern
        self.start = 0
        # per tokenizer OBJECT, weakly: an id() could be reused by another
        # tokenizer after the first one is collected
        self._tables = weakref.WeakKeyDictionary()

    @property
    def n_states(self) -> int:
        return int(self.trans.shape[0])

    @classmethod
    def from_regex(cls, pattern: str, max_states: int = MAX_STATES,
                   seconds: float | None = None) -> "Grammar":
        """max_states bounds the result AND, through it, the work spent on
        the way (NFA size, subset construction); `seconds` adds a wall-clock
        budget.  Exceeding either is a ValueError."""
        max_states = min(int(max_states), MAX_STATES)
        budget = _Budget(max_states, seconds)
        ast = _Parser(pattern).parse()
        nfa = _NFA(budget)
        s, e = nfa.build(ast)
        trans, acc = _determinise(nfa, s, e, max_states)
        trans, acc = _trim_minimise(trans, acc, budget)
        if trans.shape[0] > max_states:
            raise ValueError(f"pattern too large: {trans.shape[0]} automaton "
                             f"states, the limit is {max_states}")
        return cls(trans, acc, pattern)

    @classmethod
    def json_object(cls, fields, max_states: int = MAX_STATES) -> "Grammar":
        return cls.from_regex(json_object_regex(fields), max_states)

    # ---- matching on the host (tests, validation)
    def walk(self, state: int, data: bytes) -> int:
        for b in data:
            if state < 0:
                return -1
            state = int(self.trans[state, b])
        return state

    def matches(self, data) -> bool:
        if isinstance(data, str):
            data = data.encode("utf-8")
        s = self.walk(0, data)
        return s >= 0 and bool(self.accepting[s])

    # ---- token tables
    def token_tables(self, tokenizer) -> TokenTables:
        hit = self._tables.get(tokenizer)
        if hit is not None:
            return hit
        t0 = time.perf_counter()
        n = self.n_states
        if n > MAX_STATES:
            raise ValueError(f"{n} automaton states, the limit is "
                             f"{MAX_STATES}")
        N = n + 1
        done = n
        Vt = int(tokenizer.vocab_size)
        tb = getattr(tokenizer, "token_bytes", None)
        if tb is None:        # the byte tokenizer: ids 3..258 are raw bytes
            tb = [b""] * 3 + [bytes([b]) for b in range(256)]
        lens = np.fromiter((len(b) for b in tb), dtype=np.int64, count=Vt)
        L = int(lens.max())
        tbytes = np.zeros((Vt, L), dtype=np.int64)
        for t, b in enumerate(tb):
            if b:
                tbytes[t, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        # rows n (DONE) and n + 1 (dead) never leave the dead state
        dead = n + 1
        ext = np.full((n + 2, 256), dead, dtype=np.int32)
        ext[:n] = np.where(self.trans >= 0, self.trans, dead)
        cur = np.repeat(np.arange(N, dtype=np.int32)[:, None], Vt, axis=1)
        cur[done] = dead
        for pos in range(L):
            live = lens > pos
            cols = np.flatnonzero(live)
            cur[:, cols] = ext[cur[:, cols], tbytes[cols, pos][None, :]]
        nxt = np.where(cur == dead, -1, cur).astype(np.int16)
        nxt[:, lens == 0] = -1
        nxt[:, [PAD_ID, BOS_ID]] = -1
        nxt[:, EOS_ID] = -1
        nxt[np.flatnonzero(self.accepting), EOS_ID] = done
        nxt[done, EOS_ID] = done
        mask = pack_mask(nxt)
        # dist: BFS backwards over the distinct (state, successor) edges
        src, tok = np.nonzero(nxt >= 0)
        dst = nxt[src, tok].astype(np.int64)
        edges = np.unique(src.astype(np.int64) * N + dst)
        e_src, e_dst = edges // N, edges % N
        INF = np.iinfo(np.int16).max
        dist = np.full(N, INF, dtype=np.int64)
        dist[done] = 0
        dist[:n][self.accepting] = 0
        d = 0
        while True:
            hit_src = e_src[(dist[e_dst] == d)]
            hit_src = hit_src[dist[hit_src] == INF]
            if hit_src.size == 0:
                break
            d += 1
            dist[hit_src] = d
        assert (dist < INF).all(), "a live state cannot reach acceptance"
        assert (nxt[:n] >= 0).any(axis=1).all(), \
            "a live state has no allowed token"
        tables = TokenTables(np.ascontiguousarray(nxt), mask,
                             dist.astype(np.int16), 0,
                             time.perf_counter() - t0)
        self._tables[tokenizer] = tables
        return tables


# ---------------------------------------------------------------- JSON
_JSON_STRING = (r'"([^"\\\x00-\x1f]|\\(["\\/bfnrt]|u[0-9a-fA-F]{4}))*"')
_JSON_INT = r"-?(0|[1-9][0-9]{0,17})"


def _quote(text: str) -> str:
    """A JSON string literal as a regex that matches exactly it."""
    import json

    lit = json.dumps(str(text), ensure_ascii=False)
    return "".join("\\" + c if c in _SPECIAL else c for c in lit)


def json_object_regex(fields) -> str:
    """Regex of a JSON object with the given fields in the given order.

    fields: a list of dicts {"name": str, "type": t, ...} with t one of
    "enum" (with "values": [str, ...]), "boolean", "integer", "string",
    "array" (of strings, with "max_items": n >= 0).  "optional": true is
    allowed on the LAST field only.  At most one space after ':' and ','."""
    if not isinstance(fields, (list, tuple)):
        raise ValueError("fields must be a list of field descriptions")
    parts = []
    for i, f in enumerate(fields):
        if not isinstance(f, dict) or "name" not in f or "type" not in f:
            raise ValueError("every field needs a name and a type")
        t = f["type"]
        if t == "enum":
            vals = f.get("values")
            if not vals or not all(isinstance(v, str) for v in vals):
                raise ValueError("an enum field needs string values")
            val = "(" + "|".join(_quote(v) for v in vals) + ")"
        elif t == "boolean":
            val = "(true|false)"
        elif t == "integer":
            val = _JSON_INT
        elif t == "string":
            val = _JSON_STRING
        elif t == "array":
            m = int(f.get("max_items", 0))
            if m < 0 or m > 64:
                raise ValueError("max_items must be in [0, 64]")
            if m == 0:
                val = r"\[\]"
            elif m == 1:
                val = r"\[(" + _JSON_STRING + r")?\]"
            else:
                val = (r"\[(" + _JSON_STRING + "(, ?" + _JSON_STRING
                       + "){0,%d})?" % (m - 1) + r"\]")
        else:
            raise ValueError(f"unsupported field type {t!r}")
        item = _quote(f["name"]) + ": ?" + val
        if f.get("optional"):
            if i != len(fields) - 1:
                raise ValueError("only the last field may be optional")
            parts.append(("opt", item))
        else:
            parts.append(("req", item))
    body = ""
    for i, (kind, item) in enumerate(parts):
        sep = ", ?" if i else ""
        if kind == "opt":
            body += "(" + sep + item + ")?"
        else:
            body += sep + item
    return r"\{" + body + r"\}"


VERDICT_FIELDS = [
    {"name": "verdict", "type": "enum", "values": ["pass", "warn", "fail"]},
    {"name": "citations_ok", "type": "boolean"},
    {"name": "notes", "type": "array", "max_items": 4},
    {"name": "revised_answer", "type": "string", "optional": True},
]
VERDICT_GRAMMAR = Grammar.json_object(VERDICT_FIELDS)
