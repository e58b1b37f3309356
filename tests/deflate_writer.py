"""A test-side DEFLATE writer (RFC 1951 inside the RFC 1950 wrapper) and a catalogue of LEGAL streams that a normal
compressor may never emit: code lengths at and beyond what the decoder's lookup tables hold, every length / distance
symbol with its extra bits all 0 and all 1, overlapping copies, copies across the decoder's flush and window boundaries,
empty and one-symbol blocks, dynamic headers with chosen HLIT / HDIST / HCLEN and chosen 16 / 17 / 18 runs, headers and
matches placed across the decoder's input-ring halves, every CINFO and FLEVEL, and random streams.

Written from the two RFCs in plain Python; it shares no text with nemoflux_amd/csrc/nf_inflate_core.h and uses nothing of
zlib but adler32.  `Stream.data` is what the writer INTENDS a stream to hold; the reference of every test is
zlib.decompress (tests/test_inflate_cpu.py pins the two against each other).

Tokens: an int 0..255 is a literal, (length, distance) a match, (length, distance, lsym) a match whose length is written
with length symbol lsym (258 as 284 + 31).

Two demands of the catalogue cannot be met by a legal stream, for reasons of the format:
  * HCLEN = 4 code-length codes describes only 16, 17, 18 and 0: every length is then 0 and there is no end-of-block code.
    The smallest legal count is 5 (lengths 0 and 8); 'hclen_5', 'hclen_8' (the field value 4) and 'hclen_19' are present.
  * a 16-run of r repeats after a length v needs r + 1 codes of length v in a row; the literal and the distance set hold
    at most 2^v each, so after v = 1 only r = 3 exists (two literal / length codes + two distance codes, across the
    boundary).  Every other pair (v, r) is present.
"""
import functools
import heapq
import zlib

import numpy

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 30


class BitWriter(object):
    """bits go out least significant first (RFC 1951 3.1.1); Huffman codes most significant bit first"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    @property
    def nbits(self):
        return 8 * len(self.out) + self.n

    def bits(self, value, n):
        assert 0 <= value < (1 << n)
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def huff(self, code, n):
        assert n > 0
        self.bits(int(format(code, '0%db' % n)[::-1], 2), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)


def canonical_codes(lengths):
    """RFC 1951 3.2.2: the code of every symbol from the code lengths (None where the length is 0)"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for bits in range(1, 17):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = []
    for l in lengths:
        if l:
            out.append(nxt[l])
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lengths):
    """sum of 2^-l in units of 2^-15: 32768 = complete"""
    return sum(1 << (15 - l) for l in lengths if l)


def lengths_from_freqs(freqs, maxbits):
    """Huffman code lengths of the symbols with a frequency, limited to maxbits and made complete by a Kraft repair"""
    used = [s for s, f in enumerate(freqs) if f > 0]
    lens = [0] * len(freqs)
    if len(used) == 1:
        lens[used[0]] = 1
    if len(used) < 2:
        return lens
    heap = [(freqs[s], s, (s,)) for s in used]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], min(a[1], b[1]), a[2] + b[2]))
    for s in used:
        lens[s] = min(lens[s], maxbits)
    unit = lambda l: 1 << (maxbits - l)
    total = sum(unit(lens[s]) for s in used)
    while total > unit(0):                     # over-subscribed by the limit: lengthen the longest code that can be
        s = max((s for s in used if lens[s] < maxbits), key=lambda s: (lens[s], -freqs[s]))
        total -= unit(lens[s]) - unit(lens[s] + 1)
        lens[s] += 1
    while total < unit(0):                     # left over: shorten the longest code that fits the gap
        gap = unit(0) - total
        s = max((s for s in used if unit(lens[s]) <= gap), key=lambda s: (lens[s], freqs[s]))
        total += unit(lens[s])
        lens[s] -= 1
    return lens


def stair(nsym_total, order):
    """lengths 1, 2, ..., n-1, n-1 for the n symbols of `order` (a complete code; n = 16 uses every length 1..15)"""
    lens = [0] * nsym_total
    n = len(order)
    assert 2 <= n <= 16 and len(set(order)) == n
    for k, s in enumerate(order):
        lens[s] = min(k + 1, n - 1)
    return lens


def flat(nsym_total, symbols):
    """a complete code of two adjacent lengths over `symbols` (the first ones get the shorter)"""
    n = len(symbols)
    assert n >= 2
    b = (n - 1).bit_length()
    nshort = (1 << b) - n
    lens = [0] * nsym_total
    for k, s in enumerate(symbols):
        lens[s] = b - 1 if k < nshort else b
    return lens


def length_symbol(length):
    if length == 258:
        return 28
    return max(i for i in range(28) if LEN_BASE[i] <= length)


def distance_symbol(dist):
    return max(i for i in range(30) if DIST_BASE[i] <= dist)


def expand(tokens, out):
    """append to `out` (bytearray, holding the history) the bytes the tokens stand for: the writer's intent"""
    for t in tokens:
        if isinstance(t, tuple):
            length, dist = t[0], t[1]
            assert 3 <= length <= 258 and 1 <= dist <= 32768 and dist <= len(out), t
            for _ in range(length):
                out.append(out[-dist])
        else:
            out.append(t)
    return out


def zero_ops(n):
    """n zero lengths by the longest runs"""
    ops = []
    while n:
        if n >= 11:
            r = min(n, 138)
            ops.append((18, r))
        elif n >= 3:
            r = n
            ops.append((17, r))
        else:
            r = 1
            ops.append((0, 1))
        n -= r
    return ops


def header_ops(seq, mode='greedy', rng=None, nlit=None):
    """the code-length sequence (literal / length lengths followed by the distance lengths) as (symbol, count) operations.
    'plain': no runs; 'greedy': the longest runs, also across the literal / distance boundary; 'split': the longest runs
    that stay on one side of it (index nlit); 'random': any legal choice, random repeat counts"""
    ops, i, n = [], 0, len(seq)
    while i < n:
        v = seq[i]
        run = 1
        lim = nlit if (mode == 'split' and i < nlit) else n
        while i + run < lim and seq[i + run] == v:
            run += 1
        opts = [(v, 1)]
        if mode != 'plain':
            if v == 0 and run >= 3:
                opts += [(17, r) for r in range(3, min(run, 10) + 1)]
                opts += [(18, r) for r in range(11, min(run, 138) + 1)]
            if i > 0 and seq[i - 1] == v and run >= 3 and not (mode == 'split' and i == nlit):
                opts += [(16, r) for r in range(3, min(run, 6) + 1)]
        if mode == 'random':
            op = opts[int(rng.integers(len(opts)))] if rng.random() < 0.7 else opts[-1]
        else:
            op = max(opts, key=lambda o: (o[1], o[0]))
        ops.append(op)
        i += op[1]
    return ops


def ops_expand(ops):
    seq = []
    for sym, cnt in ops:
        if sym < 16:
            assert cnt == 1
            seq.append(sym)
        elif sym == 16:
            assert 3 <= cnt <= 6 and seq
            seq += [seq[-1]] * cnt
        elif sym == 17:
            assert 3 <= cnt <= 10
            seq += [0] * cnt
        else:
            assert sym == 18 and 11 <= cnt <= 138
            seq += [0] * cnt
    return seq


class Stream(object):
    """one zlib stream under construction; .data collects the bytes it is meant to decode to"""

    def __init__(self):
        self.w = BitWriter()
        self.data = bytearray()
        self.closed = False
        self.marks = []           # absolute bit offsets (zlib header included) of the tokens of the last Huffman block

    def _begin(self, final, btype):
        assert not self.closed
        self.closed = bool(final)
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, payload, final=False):
        payload = bytes(payload)
        assert len(payload) <= 65535
        self._begin(final, 0)
        self.w.align()
        self.w.bits(len(payload), 16)
        self.w.bits(len(payload) ^ 0xffff, 16)
        self.w.out += payload
        self.data += payload
        return self

    def _tokens(self, tokens, litlens, distlens):
        lc, dc = canonical_codes(litlens), canonical_codes(distlens)
        w = self.w
        self.marks = []
        for t in tokens:
            self.marks.append(16 + w.nbits)
            if isinstance(t, tuple):
                length, dist = t[0], t[1]
                ls = (t[2] - 257) if len(t) > 2 else length_symbol(length)
                assert 0 <= length - LEN_BASE[ls] < (1 << LEN_EXTRA[ls]) and litlens[257 + ls], t
                w.huff(lc[257 + ls], litlens[257 + ls])
                w.bits(length - LEN_BASE[ls], LEN_EXTRA[ls])
                ds = distance_symbol(dist)
                assert distlens[ds], t
                w.huff(dc[ds], distlens[ds])
                w.bits(dist - DIST_BASE[ds], DIST_EXTRA[ds])
            else:
                assert litlens[t], t
                w.huff(lc[t], litlens[t])
        w.huff(lc[256], litlens[256])
        expand(tokens, self.data)

    def fixed(self, tokens, final=False):
        self._begin(final, 1)
        self._tokens(tokens, FIXED_LIT, FIXED_DIST)
        return self

    def dynamic(self, tokens, litlens=None, distlens=None, final=False, hlit=None, hdist=None, hclen=None, runs='greedy',
                ops=None, rng=None):
        """litlens / distlens: explicit code lengths (default: Huffman lengths of the tokens' own frequencies); hlit / hdist:
        how many of them the header carries (default: up to the last one in use); hclen: how many code-length code lengths
        (default: as few as possible); runs: see header_ops; ops: the header's run operations, spelled out"""
        if litlens is None or distlens is None:
            lf, df = [0] * 286, [0] * 30
            lf[256] = 1
            for t in tokens:
                if isinstance(t, tuple):
                    lf[(t[2] if len(t) > 2 else 257 + length_symbol(t[0]))] += 1
                    df[distance_symbol(t[1])] += 1
                else:
                    lf[t] += 1
            litlens = lengths_from_freqs(lf, 15) if litlens is None else litlens
            distlens = lengths_from_freqs(df, 15) if distlens is None else distlens
        litlens, distlens = list(litlens), list(distlens)
        litlens += [0] * (286 - len(litlens))
        distlens += [0] * (30 - len(distlens))
        assert len(litlens) == 286 and len(distlens) == 30 and litlens[256]
        for lens in (litlens, distlens):
            used = [l for l in lens if l]
            assert kraft(lens) == 32768 or used in ([], [1]) or (lens is distlens and used == [1]), 'not a legal code'
        if hlit is None:
            hlit = max(257, 1 + max(s for s in range(286) if litlens[s]))
        if hdist is None:
            hdist = max([1] + [1 + s for s in range(30) if distlens[s]])
        assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and not any(litlens[hlit:]) and not any(distlens[hdist:])
        seq = litlens[:hlit] + distlens[:hdist]
        if ops is None:
            ops = header_ops(seq, runs, rng, hlit)
        assert ops_expand(ops) == seq, 'the run operations do not spell the code lengths'
        cf = [0] * 19
        for sym, _ in ops:
            cf[sym] += 1
        if sum(1 for f in cf if f) == 1:          # the code-length code must be complete: a second, unused code
            cf[0 if cf[0] == 0 else 18] += 1
        cl = lengths_from_freqs(cf, 7)
        need = max(4, 1 + max(k for k in range(19) if cl[CL_ORDER[k]]))
        hclen = need if hclen is None else hclen
        assert need <= hclen <= 19
        cc = canonical_codes(cl)
        w = self.w
        self._begin(final, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for k in range(hclen):
            w.bits(cl[CL_ORDER[k]], 3)
        for sym, cnt in ops:
            w.huff(cc[sym], cl[sym])
            if sym == 16:
                w.bits(cnt - 3, 2)
            elif sym == 17:
                w.bits(cnt - 3, 3)
            elif sym == 18:
                w.bits(cnt - 11, 7)
        self._tokens(tokens, litlens, distlens)
        return self

    def finish(self, cinfo=7, flevel=2):
        """RFC 1950: CMF, FLG (FCHECK makes the pair a multiple of 31), the blocks, Adler-32 big-endian"""
        assert self.closed and 0 <= cinfo <= 7 and 0 <= flevel <= 3
        self.w.align()
        cmf = (cinfo << 4) | 8
        flg = flevel << 6
        flg |= (31 - ((cmf << 8) | flg) % 31) % 31
        return bytes([cmf, flg]) + bytes(self.w.out) + (zlib.adler32(bytes(self.data)) & 0xffffffff).to_bytes(4, 'big')


# ------------------------------------------------------------------------------------------------------------- the catalogue
SIZES = (2048, 16384, 70000, 140000)      # decoded lengths the cases are padded to: a handful of device launches


def _rand(rng, n, lo=0, hi=256):
    return [int(x) for x in rng.integers(lo, hi, n)]


def _history(s, rng, nbytes, period=300):
    """cheap history with content: `period` random stored bytes, then fixed-code copies of them up to nbytes"""
    s.stored(bytes(_rand(rng, period)))
    toks = []
    left = nbytes - period
    while left >= 3:
        n = min(258, left)
        toks.append((n, period))
        left -= n
    s.fixed(toks + [7] * left)
    return s


def _close(s, last='pad', rng=None, cinfo=7, flevel=2):
    """pad to one of SIZES with stored blocks of random bytes, then the last block"""
    size = min(z for z in SIZES if z >= len(s.data))
    pad = size - len(s.data)
    rng = rng or numpy.random.default_rng(len(s.data))
    while pad > 65535 or (pad and last != 'pad'):
        n = min(pad, 65535)
        s.stored(rng.integers(0, 256, n, dtype=numpy.uint8).tobytes())
        pad -= n
    if last == 'pad':
        s.stored(rng.integers(0, 256, pad, dtype=numpy.uint8).tobytes(), final=True)
    elif last == 'empty_stored':
        s.stored(b'', final=True)
    elif last == 'empty_fixed':
        s.fixed([], final=True)
    else:
        assert last == 'empty_dynamic'
        s.dynamic([], final=True)
    return s.finish(cinfo, flevel), bytes(s.data)


def _run16_block(s, v, r):
    """a dynamic block whose header holds `v, 16 x r`: r + 1 codes of length v in a row, in the literal / length set when
    that leaves room for an end-of-block code, else across the boundary into the distance set"""
    total = r + 1
    cap = 1 << v

    def rest(units, first_free, limit):     # fill what is left of a code space (units of 2^-15) with single codes
        lens = {}
        sym = first_free
        for l in range(1, 16):
            if units & (1 << (15 - l)):
                assert sym < limit
                lens[sym] = l
                sym += 1
        return lens
    lit, dist = [0] * 286, [0] * 30
    if total <= cap - 1:
        a, b = total, 0
        first = 256 - a
        for k in range(a):
            lit[first + k] = v
        for sym, l in rest(32768 - a * (1 << (15 - v)), 256, 286).items():
            lit[sym] = l
        dist[0] = 1
        ndist = 1
        toks = list(range(first, 256))
    else:
        a = cap
        b = total - a
        assert b <= cap
        first = 257 - a
        for k in range(a):
            lit[first + k] = v
        for k in range(b):
            dist[k] = v
        fill = rest(32768 - b * (1 << (15 - v)), b, 30) if b else {0: 1}
        for sym, l in fill.items():
            dist[sym] = l
        ndist = 1 + max(k for k in range(30) if dist[k])
        toks = list(range(first, 256))
    nlit = 1 + max(k for k in range(286) if lit[k])
    nlit = max(nlit, 257)
    seq = lit[:nlit] + dist[:ndist]
    ops = zero_ops(first) + [(v, 1), (16, r)] + [(x, 1) for x in seq[first + total:]]
    s.dynamic(toks, lit, dist, hlit=nlit, hdist=ndist, ops=ops)


def _build_catalogue():
    cat = {}
    R = lambda k: numpy.random.default_rng(1000 + k)

    def add(name, s, **kw):
        assert name not in cat
        cat[name] = _close(s, **kw)

    # ---- a. code lengths
    lits16 = [65 + k for k in range(15)] + [256]                              # 'A'..'O' then EOB: lengths 1..15, 15
    rng = R(1)
    s = Stream()
    s.dynamic([lits16[int(k)] for k in rng.integers(0, 15, 600)] + lits16[:15] * 3, stair(286, lits16), [0] * 30)
    add('a_literal_lengths_1_to_15_eob_15', s)
    s = Stream()
    order = [256] + [65 + k for k in range(15)]                                # EOB 1 bit, literals 2..15, 15
    s.dynamic([order[1 + int(k)] for k in rng.integers(0, 15, 400)] + order[1:] * 2, stair(286, order), [0] * 30)
    add('a_literal_lengths_eob_1', s)
    s = Stream()
    _history(s, rng, 400)
    order = [97, 98, 99, 100, 101, 102, 103, 104, 105, 256, 257, 265, 273, 281, 284, 285]   # length codes of 11..15 bits
    dl = stair(30, [0, 5, 10, 16])
    toks = []
    for k in range(60):
        toks += [order[int(rng.integers(0, 9))], ([3, 11, 12, 35, 42, 131, 162, 227, 257, 258][k % 10], [1, 7, 8, 33, 48, 257, 384][k % 7])]
    toks.append((258, 300, 284))
    s.dynamic(toks, stair(286, order), dl)
    add('a_length_codes_11_to_15_bits', s)
    s = Stream()
    _history(s, rng, 33000)
    dorder = [0, 3, 4, 7, 8, 11, 12, 15, 16, 19, 20, 23, 24, 27, 28, 29]       # distance codes of 1..15, 15 bits
    toks = []
    for k in range(160):
        ds = dorder[k % 16]
        x = [0, (1 << DIST_EXTRA[ds]) - 1, int(rng.integers(0, 1 << DIST_EXTRA[ds]))][(k // 16) % 3]
        toks += [(int(rng.integers(3, 40)), DIST_BASE[ds] + x), int(rng.integers(0, 256))]
    s.dynamic(toks, None, stair(30, dorder))
    add('a_distance_lengths_1_to_15', s)
    s = Stream()
    lit = [0] * 286
    lit[120] = lit[256] = 1
    s.dynamic([120] * 777, lit, [0] * 30)
    add('a_two_one_bit_codes', s)
    s = Stream()
    for n in (2, 3, 4, 5):                                                     # 2^n codes of n bits: pairs of n + n bits
        syms = list(range(40, 40 + (1 << n) - 1)) + [256]
        s.dynamic([syms[int(k)] for k in rng.integers(0, len(syms) - 1, 500)], flat(286, syms), [0] * 30)
    syms = [10, 11, 12, 13, 256, 14, 15, 16, 17, 18]                           # mixed 1..5 + 5..1 bit pairs, odd + even totals
    s.dynamic([syms[int(k)] for k in rng.integers(0, 10, 800) if syms[int(k)] != 256], stair(286, syms), [0] * 30)
    add('a_pairs_of_short_literal_codes', s)
    s = Stream()
    _history(s, rng, 400)
    order = [97, 98, 257, 256, 99, 100, 270, 101, 102, 88, 89, 285, 103, 260, 104, 105]   # 'X' = 88: 10 bits, 'Y' = 89: 11 bits
    ll, dl = stair(286, order), stair(30, [2, 9, 0])
    kinds = [[97], [98, 97], [88], [89], [105], [(3, 3)], [(258, 30)], [(6, 1)], None]
    for first in (88, 89):
        toks = []
        for kind in kinds:
            if kind is None:                  # ... followed by the end of the block
                s.dynamic(toks + [first], ll, dl)
                toks = []
            else:
                toks += [first] + kind
        s.dynamic(toks, ll, dl)
    add('a_literal_codes_of_10_and_11_bits', s)

    # ---- b. symbols
    def every_length_symbol():
        toks = []
        for ls in range(29):
            for x in (0, (1 << LEN_EXTRA[ls]) - 1):
                toks += [int(rng.integers(0, 256)), (LEN_BASE[ls] + x, int(rng.integers(1, 400)), 257 + ls)]
        return toks + [(258, 77, 284)]

    def every_distance_symbol(pos):
        toks = []
        for ds in range(30):
            for x in (0, (1 << DIST_EXTRA[ds]) - 1):
                toks += [(int(rng.integers(3, 12)), DIST_BASE[ds] + x), int(rng.integers(0, 256))]
        return toks
    allsym = list(range(286))
    for kind in ('fixed', 'dynamic'):
        s = Stream()
        _history(s, rng, 400)
        t = every_length_symbol()
        s.fixed(t) if kind == 'fixed' else s.dynamic(t, flat(286, allsym), flat(30, list(range(30))))
        add('b_every_length_symbol_' + kind, s)
        s = Stream()
        _history(s, rng, 32768)
        t = [(5, 32768)] + every_distance_symbol(len(s.data))       # distance 32768 at position 32768 = the position itself
        s.fixed(t) if kind == 'fixed' else s.dynamic(t, flat(286, allsym), flat(30, list(range(30))))
        add('b_every_distance_symbol_' + kind, s)
    s = Stream()
    s.stored(bytes(_rand(rng, 9)))
    s.fixed([(4, 9), (9, 13), (258, 22)])                           # distance = position, three times
    add('b_distance_equal_to_position', s)
    s = Stream()
    _history(s, rng, 33000, period=997)
    order = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 256, 281, 282]         # 15-bit length codes with 5 extra bits
    dorder = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29]            # 15-bit distance codes with 13 extra bits
    toks = [([131, 162, 163, 194][k % 4], [16385, 24576, 24577, 32768][(k // 2) % 4] - (k % 3)) for k in range(120)]
    toks = [(l, min(max(d, 16385), 32768)) for l, d in toks]
    s.dynamic(toks, stair(286, order), stair(30, dorder))
    add('b_48_bit_matches_back_to_back', s)

    # ---- c. copies
    dists = [1, 2, 3, 4, 7, 8, 31, 32, 33, 63, 64, 65, 66]
    lens = [3, 4, 63, 64, 65, 257, 258]
    for kind in ('fixed', 'dynamic'):
        s = Stream()
        toks = _rand(rng, 70)
        for d in dists + [5, 16, 48]:
            for l in lens + [int(rng.integers(5, 258))]:
                toks += [(l, d), int(rng.integers(0, 256))]
        s.fixed(toks) if kind == 'fixed' else s.dynamic(toks)
        add('c_overlapping_copies_' + kind, s)
    s = Stream()
    toks, pos = [], 0
    for B in [8192 * k for k in range(1, 9)]:                      # every flush edge; 32768 and 65536 are the window's too
        # destinations across B - 1 / B / B + 1, then sources across the same bytes
        fill = B - 276 - pos
        toks += _rand(rng, fill)
        pos += fill
        for ln, d in ((258, min(pos, 32768)), (9, 5), (6, 300)):   # ends at B - 3 ...
            toks.append((ln, d))
            pos += ln
        toks.append((10, min(pos, 32768) if B >= 32768 else 1000))   # ... and this one covers B - 3 .. B + 6
        pos += 10
        toks += _rand(rng, 3)
        pos += 3
        toks.append((12, pos - (B - 6)))                           # source B - 6 .. B + 5
        pos += 12
        toks.append((258, pos - (B - 100)))                        # source B - 100 .. B + 157
        pos += 258
    s.dynamic(toks)
    add('c_copies_across_flush_and_window_edges', s)

    # ---- d. blocks
    s = Stream()
    s.stored(b'')
    s.fixed(_rand(rng, 50))
    s.stored(b'')
    s.dynamic(_rand(rng, 50, 0, 9))
    s.stored(b'')
    s.stored(b'')
    add('d_empty_stored_first_middle_last', s, last='empty_stored')
    s = Stream()
    s.stored(bytes(_rand(rng, 65535)))
    s.fixed([1, 2, 3])
    add('d_stored_65535', s)
    s = Stream()
    phases = set()
    for p in range(8):
        s.fixed([200] * p + [3])                                   # nine-bit literals move the end by one bit each
        phases.add(s.w.nbits % 8)
        s.stored(bytes(_rand(rng, 5 + p)))
    assert len(phases) == 8
    add('d_stored_behind_every_bit_phase', s)
    s = Stream()
    s.fixed([])
    s.dynamic([])
    s.fixed(_rand(rng, 20))
    s.dynamic([])
    s.fixed([])
    add('d_empty_fixed_and_dynamic', s, last='empty_dynamic')
    s = Stream()
    s.dynamic(_rand(rng, 2048, 0, 40))
    add('d_final_empty_block_behind_the_data', s, last='empty_fixed')
    s = Stream()
    for k in range(1000):
        b = int(rng.integers(0, 256))
        [lambda: s.stored(bytes([b])), lambda: s.fixed([b]), lambda: s.dynamic([b])][k % 3]()
    add('d_1000_one_literal_blocks', s)
    s = Stream()
    s.dynamic(_rand(rng, 300, 0, 30), None, [0] * 30, hdist=1)
    add('d_no_distance_code', s)
    s = Stream()
    _history(s, rng, 400)
    dl = [0] * 30
    dl[6] = 1
    s.dynamic([x for k in range(40) for x in (int(rng.integers(0, 256)), (3 + k, 9 + k % 4))], None, dl)
    add('d_one_one_bit_distance_code', s)
    s = Stream()
    _history(s, rng, 400)
    s.dynamic(every_length_symbol(), flat(286, allsym), flat(30, list(range(30))), hlit=286, hdist=30, runs='plain')
    add('d_hlit_286_hdist_30', s)
    for hclen, syms in ((5, list(range(1, 257))), (8, None), (19, None)):
        s = Stream()
        if hclen == 5:                      # lengths 0 and 8 only: the code-length codes 16, 17, 18, 0, 8
            s.dynamic(_rand(rng, 200, 1, 256), flat(286, syms), [0] * 30, hclen=5, runs='greedy')
        elif hclen == 8:                    # ... and 7, 9, 6
            ll = flat(286, list(range(20, 257)))
            assert set(ll) <= {0, 6, 7, 8, 9}
            s.dynamic(_rand(rng, 200, 20, 256), ll, [0] * 30, hclen=8)
        else:
            s.dynamic(_rand(rng, 200, 0, 9), None, [0] * 30, hclen=19)
        add('d_hclen_%d' % hclen, s)

    # ---- e. header runs
    s = Stream()
    for v in range(1, 16):
        for r in (3, 4, 5, 6):
            if v == 1 and r > 3:
                continue                     # would need more than 2 + 2 one-bit codes
            _run16_block(s, v, r)
    add('e_16_runs_after_every_length', s)
    s = Stream()
    lit = stair(286, [0, 4, 15, 27, 166, 256])       # gaps of 3, 10, 11, 138 zero lengths (and 89)
    s.dynamic([0, 4, 15, 27, 166] * 9, lit, [0] * 30)
    add('e_17_and_18_runs_shortest_and_longest', s)
    s = Stream()
    _history(s, rng, 400)
    lit = stair(286, [50, 51, 52, 256, 257])
    dl = [0] * 30
    dl[10] = 1
    s.dynamic([50, 51, (3, 33), 52, (3, 48)], lit, dl, hlit=286, hdist=11)   # zeros 258..285 and 0..9: one 18 of 38
    assert (18, 38) in header_ops(lit[:286] + dl[:11])
    s.dynamic([253, 254, 255], [0] * 253 + [2, 2, 2, 2], [2, 2, 1], hlit=257, hdist=3,
              ops=zero_ops(253) + [(2, 1), (16, 5), (1, 1)])                  # 2, then 16 x 5 over 254..256 and distances 0, 1
    add('e_runs_across_the_literal_distance_boundary', s)

    # ---- f. input ring (halves of 512 bytes; the stream may start 0..3 bytes into a word)
    for edge in (512, 1024):
        s = Stream()
        s.stored(bytes(_rand(rng, edge - 2 - 5 - 20)))                        # the header starts 20 bytes before the edge ...
        start = 2 + len(s.w.out)
        s.dynamic(_rand(rng, 300), flat(286, list(range(257))), [0] * 30, runs='plain')
        assert start < edge - 8 and s.marks[0] // 8 > edge + 8                # ... and ends behind it, whatever the alignment
        add('f_dynamic_header_across_offset_%d' % edge, s)
        for byte in range(edge - 4, edge):
            order = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 256, 281, 282]
            dorder = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 28, 29]
            toks = [1, 2, (150, 16400), (162, 16385), 3, (131, 16390)]
            pad = 100
            for attempt in (0, 1):
                s = Stream()
                _history(s, R(byte), 16500, period=61)
                s.stored(bytes(_rand(R(byte + 1), pad)))
                s.dynamic(toks, stair(286, order), stair(30, dorder))
                pad += byte - s.marks[2] // 8
            assert s.marks[2] // 8 == byte and s.marks[3] - s.marks[2] == 48
            add('f_48_bit_match_from_byte_%d' % byte, s)

    # ---- g. wrapper
    for cinfo in range(8):
        s = Stream()
        win = 1 << (cinfo + 8)
        toks = _rand(rng, win)
        for k in range(30):
            toks += [(int(rng.integers(3, 259)), [win, win - 1, 1, win // 2][k % 4]), int(rng.integers(0, 256))]
        s.dynamic(toks) if cinfo % 2 else s.fixed(toks)
        add('g_cinfo_%d' % cinfo, s, cinfo=cinfo)
    for flevel in range(4):
        s = Stream()
        s.dynamic(_rand(rng, 500, 0, 20))
        add('g_flevel_%d' % flevel, s, flevel=flevel)
    return cat


@functools.lru_cache(maxsize=None)
def _catalogue():
    return _build_catalogue()


def foreign_streams():
    """{name: (zlib stream, the bytes the writer means it to hold)}; every decoded length is one of SIZES"""
    return dict(_catalogue())


# ------------------------------------------------------------------------------------------------------------- random streams
RANDOM_SIZE = 12000


def _random_stream(rng, size):
    s = Stream()
    alpha = rng.choice(256, int(rng.integers(1, 257)), replace=False)
    weights = rng.random(alpha.size) ** int(rng.integers(1, 9))            # skewed
    weights /= weights.sum()
    target = int(rng.integers(1, size - 600))
    while len(s.data) < target:
        toks, pos = [], len(s.data)
        for _ in range(int(rng.integers(1, 400))):
            if pos and rng.random() < 0.4:
                d = int(min(pos, 32768, 1 + rng.integers(0, 1 << int(rng.integers(1, 16)))))
                l = int(min(258, 3 + rng.integers(0, 1 << int(rng.integers(1, 9)))))
                toks.append((l, d, 284) if l == 258 and rng.random() < 0.5 else (l, d))
                pos += l
            else:
                toks.append(int(alpha[rng.choice(alpha.size, p=weights)]))
                pos += 1
            if pos >= target + 500:
                break
        kind = int(rng.integers(0, 4))
        if kind == 0 and pos - len(s.data) <= 65535:
            s.stored(bytes(expand(toks, bytearray(s.data))[len(s.data):]))
        elif kind == 1:
            s.fixed(toks)
        else:
            lf, df = rng.random(286) ** 6 * 3, rng.random(30) ** 6 * 3     # codes for symbols that never occur, too
            lf[lf < 1.5] = 0
            df[df < 1.5] = 0
            lf[256] += 1
            for t in toks:
                if isinstance(t, tuple):
                    lf[t[2] if len(t) > 2 else 257 + length_symbol(t[0])] += 1 + rng.random() * 20
                    df[distance_symbol(t[1])] += 1 + rng.random() * 20
                else:
                    lf[t] += 1 + rng.random() ** 4 * 1000
            s.dynamic(toks, lengths_from_freqs(list(lf), 15), lengths_from_freqs(list(df), 15),
                      runs=['plain', 'greedy', 'split', 'random'][int(rng.integers(0, 4))], rng=rng)
    pad = size - len(s.data)
    assert pad >= 0
    s.stored(rng.integers(0, 256, pad, dtype=numpy.uint8).tobytes(), final=True)
    return s.finish(7, int(rng.integers(0, 4))), bytes(s.data)


@functools.lru_cache(maxsize=None)
def _random_streams(n, seed, size):
    rng = numpy.random.default_rng(seed)
    return tuple(_random_stream(rng, size) for _ in range(n))


def random_streams(n, seed, size=RANDOM_SIZE):
    """n (stream, intended bytes) of `size` decoded bytes each: random tokens over random alphabets (matches valid by
    construction), random block cuts and types, code lengths from skewed random frequencies limited to 15 and completed by
    the Kraft repair, random run encodings of the header"""
    return list(_random_streams(n, seed, size))


def stream_of_length(size, residue, modulus=8, seed=0):
    """a legal stream of `size` decoded bytes whose compressed length is `residue` modulo `modulus`: a stored block and as
    many empty fixed blocks (ten bits each) as that takes -- to put the streams behind it at chosen offsets"""
    rng = numpy.random.default_rng(seed)
    payload = rng.integers(0, 256, size, dtype=numpy.uint8).tobytes()
    for k in range(8 * modulus):
        s = Stream()
        for lo in range(0, size, 65535):
            s.stored(payload[lo:lo + 65535])
        for _ in range(k):
            s.fixed([])
        s.fixed([], final=True)
        out = s.finish()
        if len(out) % modulus == residue:
            return out, bytes(s.data)
    raise AssertionError('no such length')
