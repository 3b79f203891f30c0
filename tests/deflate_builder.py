"""A small DEFLATE (RFC 1951) *writer* for tests, and the hand-made streams of tests/test_inflate_handmade.py: the paths of the two
inflate decoders (trgt_amd/csrc/inflate_fast.hpp, trgt_amd/csrc/inflate_dev.hip) that zlib's compressor never emits.  Plain Python, does
not load the library.  Stream writes stored / fixed / dynamic blocks from tokens (a literal int, a match (len, dist), or a Raw escape for
malformed streams); expand() is the LZ77 expansion of the same tokens, byte by byte: a reference independent of any decoder.

  python tests/deflate_builder.py --dump FILE    every case as a record  u32 n_in, u32 n_out, u8 accept, stream bytes  (accept = 1: a
  valid stream the host decoder must take; 0: malformed, or one of the classes it leaves to zlib; n_out = 1000 for malformed streams):
  the input of tests/tools/inflate_vectors_asan.cpp."""
import collections
import struct
import sys
import zlib

import numpy as np

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
# the code-length codes of the three header styles (19 entries, by symbol)
CL_PLAIN = [4] * 16 + [0, 0, 0]                 # one 4-bit code per length, no repeats
CL_RLE = [4] * 13 + [5] * 6                     # all 19 present, complete: 13/16 + 6/32
CL_WIDEST = [7] * 16 + [1, 2, 3]                # complete (1/2 + 1/4 + 1/8 + 16/128); the symbols a header without repeats uses all take 7 bits

Raw = collections.namedtuple("Raw", "table sym xval xbits")  # table "L" / "D": that symbol of the block's code, unchecked; None: xbits raw bits
Raw.__new__.__defaults__ = (0, 0)


def _sym_table(base, extra, top):
    t = [None] * (top + 1)
    for s in range(len(base)):  # (ascending: length 258 ends up with symbol 285, not 284 + 31)
        for x in range(1 << extra[s]):
            if base[s] + x <= top:
                t[base[s] + x] = (s, x, extra[s])
    return t


_LSYM = _sym_table(LEN_BASE, LEN_EXTRA, 258)
_DSYM = _sym_table(DIST_BASE, DIST_EXTRA, 32768)


def lsym(length):
    """(symbol, extra value, extra bits) of a match length 3 .. 258"""
    s, x, n = _LSYM[length]
    return s + 257, x, n


def dsym(dist):
    """(symbol, extra value, extra bits) of a match distance 1 .. 32768"""
    return _DSYM[dist]


def canonical(lens):
    """code lengths -> {symbol: (code, length)}, RFC 1951 3.2.2 (an over-subscribed set gets codes cut to their length)"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    codes = {}
    for s, l in enumerate(lens):
        if l:
            codes[s] = (nxt[l] & ((1 << l) - 1), l)
            nxt[l] += 1
    return codes


def reversed_codes(lens):
    """per symbol (code with its bits reversed: ready for an LSB-first writer, length), None for an unused symbol"""
    out = [None] * len(lens)
    for s, (c, l) in canonical(lens).items():
        out[s] = (int(format(c, "0%db" % l)[::-1], 2), l)
    return out


def kraft(lens):
    """sum of 2^-l in units of 2^-15: 32768 for a complete code"""
    return sum(1 << (15 - l) for l in lens if l)


def flat_lens(n, used):
    """a complete code over the symbols `used` (at least two) of an alphabet of n: lengths k - 1 and k"""
    used = sorted(set(used))
    k = max(1, (len(used) - 1).bit_length())
    short = (1 << k) - len(used)
    lens = [0] * n
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    assert kraft(lens) == 32768
    return lens


def rle_symbols(seq):
    """code lengths -> [(code-length symbol, extra value, extra bits, first index, count)] with 16 / 17 / 18 wherever they apply"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, j = seq[i], i
        while j < n and seq[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138); out.append((18, k - 11, 7, i, k)); i += k; run -= k
            if run >= 3:
                out.append((17, run - 3, 3, i, run)); i += run; run = 0
        else:
            out.append((v, 0, 0, i, 1)); i += 1; run -= 1
            while run >= 3:
                k = min(run, 6); out.append((16, k - 3, 2, i, k)); i += k; run -= k
        for _ in range(run):
            out.append((v, 0, 0, i, 1)); i += 1
    return out


class BitWriter:
    def __init__(self):
        self.acc = 0; self.n = 0; self.out = bytearray()

    def bits(self, v, n):  # LSB first
        self.acc |= v << self.n; self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF); self.acc >>= 8; self.n -= 8

    def code(self, rc):  # a Huffman code, already reversed
        self.bits(rc[0], rc[1])

    def flush(self):  # to the byte boundary
        if self.n:
            self.out.append(self.acc & 0xFF); self.acc = 0; self.n = 0


class Stream:
    """blocks written one after the other; .blocks keeps their tokens for expand()"""

    def __init__(self):
        self.w = BitWriter(); self.blocks = []

    def phase(self):
        return self.w.n & 7

    def bytes(self):
        w = BitWriter(); w.acc, w.n, w.out = self.w.acc, self.w.n, bytearray(self.w.out); w.flush()
        return bytes(w.out)

    def stored(self, data, final=False, length=None, nlen=None):
        """length / nlen: what the header says instead of len(data) and its complement"""
        w = self.w
        w.bits(int(final), 1); w.bits(0, 2); w.flush()
        length = len(data) if length is None else length
        w.out += struct.pack("<HH", length, (length ^ 0xFFFF) if nlen is None else nlen) + bytes(data)
        self.blocks.append(list(data))

    def _tokens(self, tokens, lc, dc, eob):
        w = self.w
        acc, n, out = w.acc, w.n, w.out
        for t in tokens:
            if type(t) is int:
                c, l = lc[t]
                acc |= c << n; n += l
            elif type(t) is tuple:
                s, x, xb = _LSYM[t[0]]
                c, l = lc[s + 257]
                acc |= c << n; n += l
                acc |= x << n; n += xb
                s, x, xb = _DSYM[t[1]]
                c, l = dc[s]
                acc |= c << n; n += l
                acc |= x << n; n += xb
            else:
                if t.table is not None:
                    c, l = (lc if t.table == "L" else dc)[t.sym]
                    acc |= c << n; n += l
                acc |= t.xval << n; n += t.xbits
            while n >= 64:
                out += (acc & 0xFFFFFFFFFFFFFFFF).to_bytes(8, "little"); acc >>= 64; n -= 64
        if eob:
            c, l = lc[256]
            acc |= c << n; n += l
        w.acc, w.n = 0, 0
        w.bits(acc, n)
        self.blocks.append(list(tokens))

    def fixed(self, tokens, final=False, eob=True):
        self.w.bits(int(final), 1); self.w.bits(1, 2)
        self._tokens(tokens, _FIXED_LC, _FIXED_DC, eob)

    def dynamic(self, tokens, lit_lens, dist_lens, final=False, header="plain", hclen=19, hlit=None, hdist=None, cl_lens=None, cl_syms=None, eob=True):
        """header: "plain" one code per length, "rle" 16 / 17 / 18 wherever they apply (across the boundary between literal and distance
        lengths too), "widest" no repeats and 7 bits per length: the longest header.  cl_lens / cl_syms [(symbol, extra value, extra
        bits)] / hlit / hdist: written as given, for malformed headers."""
        w = self.w
        seq = list(lit_lens) + list(dist_lens)
        w.bits(int(final), 1); w.bits(2, 2)
        w.bits((len(lit_lens) if hlit is None else hlit) - 257, 5); w.bits((len(dist_lens) if hdist is None else hdist) - 1, 5); w.bits(hclen - 4, 4)
        if cl_lens is None:
            cl_lens = {"plain": CL_PLAIN, "rle": CL_RLE, "widest": CL_WIDEST}[header]
        if cl_syms is None:
            cl_syms = [r[:3] for r in rle_symbols(seq)] if header == "rle" else [(l, 0, 0) for l in seq]
        for s in CL_ORDER[:hclen]:
            w.bits(cl_lens[s], 3)
        cc = reversed_codes(cl_lens)
        for s, x, xb in cl_syms:
            w.code(cc[s]); w.bits(x, xb)
        self._tokens(tokens, reversed_codes(lit_lens), reversed_codes(dist_lens), eob)


_FIXED_LC, _FIXED_DC = reversed_codes(FIXED_LIT), reversed_codes(FIXED_DIST)


def expand(tokens_per_block):
    """the LZ77 expansion, byte by byte"""
    out = bytearray()
    for tokens in tokens_per_block:
        for t in tokens:
            if type(t) is int:
                out.append(t)
            else:
                ln, dist = t
                assert 3 <= ln <= 258 and 1 <= dist <= min(len(out), 32768), (ln, dist, len(out))
                for _ in range(ln):
                    out.append(out[-dist])
    return bytes(out)


# ---- the stream of tests/test_inflate.py for the window bookkeeping of the device decoder's hand-written loop: after 25 000 stored bytes,
#      950 matches that take EXACTLY 32 bits each (an 8-bit length code + 3 extra bits, an 8-bit distance code + 13 extra bits) behind
#      0 .. 15 two-bit literals that set the phase of the bit buffer
def run_of_32_bit_matches(n_lead, rng):
    s = Stream()
    s.stored(bytes(rng.integers(0, 256, 25000, dtype=np.uint8)))
    lit = [0] * 274
    lit[65] = 1; lit[256] = 2; lit[273] = 8
    for k in range(63): lit[k] = 8                              # 1/2 + 1/4 + 64/256 = 1: a complete code
    dst = [0] * 30
    for k, l in enumerate((1, 2, 3, 4, 5, 6, 7, 8)): dst[k] = l
    dst[29] = 8
    tokens = [65] * n_lead
    for _ in range(950):
        ln = 35 + int(rng.integers(0, 8))                       # lengths 35 .. 42
        tokens.append((ln, 24577 + int(rng.integers(0, 400))))  # distances 24 577 .. 24 976
    s.dynamic(tokens, lit, dst, final=True)
    return s.bytes()


# ================================================================================================================================
# The cases.  expected: None for a stream no decoder may take (malformed, or announced_wrongly: a valid stream whose announced size is
# one byte off); else the bytes.  n_out: the announced size.  tag: a valid stream of a class the decoders leave to zlib --
# "single_litlen" (both decline), "single_dist" (the host declines, the device takes it).
Case = collections.namedtuple("Case", "name stream expected n_out tag announced_wrongly")
Case.__new__.__defaults__ = (False,)
RINGS = (2048, 4096)  # TRGT_INFL_RING is a build option: the boundaries of both


def _case(name, s, valid=True, n_out=None, tag=None):
    data = s if isinstance(s, (bytes, bytearray)) else s.bytes()
    exp = expand(s.blocks) if valid else None
    return Case(name, bytes(data), exp, (len(exp) if valid else 1000) if n_out is None else n_out, tag)


def _rand(rng, n, lo=0, hi=256):
    return rng.integers(lo, hi, n).tolist()


GEOM_LENS = (3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 49, 50, 51, 63, 64, 65, 66, 67, 257, 258)


def _geom_dists():
    d = set(range(1, 71))
    for R in RINGS:
        d |= {R - 65, R - 64, R - 63, R - 1, R, R + 1, R + 63, R + 64, R + 65}
    return sorted(d)


def family_copy_geometry():
    """1: fixed-code blocks, random literals up to a lead position, then one length at every distance, 0 .. 3 literals in between; the list
    of distances starts somewhere else in every stream, so that each meets the lead position (a ring wrap, a segment boundary) in one"""
    rng = np.random.default_rng(101)
    leads = sorted({70} | {x for R in RINGS for x in (R - 30, R + 5, 2 * R + 5)})
    dists = _geom_dists()
    cases = []
    for i, lead in enumerate(leads):
        for j, ln in enumerate(GEOM_LENS):
            toks, op = _rand(rng, lead), lead
            k = ((i * len(GEOM_LENS) + j) * 5) % len(dists)
            for m, d in enumerate(dists[k:] + dists[:k]):
                if d > op:
                    continue
                toks.append((ln, d)); toks += _rand(rng, m % 4); op += ln + m % 4
            s = Stream(); s.fixed(toks, final=True)
            cases.append(_case("geometry lead %d len %d" % (lead, ln), s))
    return cases


def _far_followers(L1, g):
    """what follows a far match (L1, D1) that wrote [p, p + L1), g literals later: (name, tokens or None for the end of the block)"""
    f = [("source ends at p", [(9, L1 + g + 9)]), ("source ends at p+1", [(9, L1 + g + 8)]), ("source starts at p+L1-1", [(3, g + 1)]),
         ("source covers the interval", [(L1 + 5, L1 + g + 5)]), ("source covers the interval up to op", [(L1 + g + 5, L1 + g + 5)]),
         ("overlap 1", [(40, 1)]), ("overlap 2", [(9, 2)]), ("overlap 3", [(10, 3)]), ("overlap L1", [(L1 + 3, L1)]), ("overlap L1 long", [(min(258, 3 * L1 + 30), L1)]),
         ("far again", [(20, 4096 + 77)]), ("far again, same source", [(L1, 4096 + L1 + g)]), ("len 258", [(258, 300)]), ("len 258 from p", [(258, L1 + g)]),
         ("end of block", None)]
    if g:
        f.append(("source starts at p+L1", [(3, g)]))
    if L1 >= 5:
        f.append(("source inside", [(L1 - 2, L1 + g - 1)]))
    return f


def family_far_copy():
    """2: the far copy in flight.  8 192 stored bytes, then per scenario a far match and its follower; `at`: p + L1 relative to a
    segment boundary of both ring sizes (None: wherever it falls, scenarios 40 literals apart)"""
    rng = np.random.default_rng(102)
    D1s = (4096, 4097, 5000, 8191, 8192)
    cases = []
    for at in (None, -1, 0, 1):
        for L1 in (3, 17, 50):
            s, toks, op, n, part = None, [], 0, 0, 0

            def close(final_name=None):
                nonlocal s, toks, part
                if toks:
                    s.fixed(toks, final=True)
                    cases.append(_case("far copy at %s L1 %d part %d" % (at, L1, part), s))
                    part += 1
                s, toks = None, []
            for g in (0, 1, 2, 3):  # (3: the only gap at which a source that starts at p + L1 does not overlap its destination)
                for name, follow in _far_followers(L1, g):
                    if s is None or op + 2048 + 700 > 65536:
                        close()
                        s = Stream(); s.stored(bytes(_rand(rng, 8192))); op = 8192
                    if at is None:
                        toks += _rand(rng, 40); op += 40
                    else:
                        target = ((op + L1 + 300) // 2048 + 1) * 2048 + at - L1  # p
                        fill = target - op
                        toks += [(258, 4096)] * (fill // 258) + _rand(rng, fill % 258); op = target
                    toks.append((L1, D1s[n % len(D1s)])); n += 1
                    toks += _rand(rng, g); op += L1 + g
                    if follow is None:
                        s.fixed(toks); toks = []
                    else:
                        toks += follow; op += sum(t[0] for t in follow)
                    toks += _rand(rng, 3); op += 3
            close()
    return cases


def family_max_reach():
    """3: distances up to 32 768 (zlib's compressor stops at 32 506)"""
    rng = np.random.default_rng(103)
    cases = []
    for d in (32506, 32507, 32767, 32768):
        s = Stream(); s.stored(bytes(_rand(rng, 32768)))
        toks = []
        for m, ln in enumerate((3, 50, 51, 64, 65, 258) * 2):
            toks.append((ln, d)); toks += _rand(rng, m % 4)
        s.fixed(toks, final=True)
        cases.append(_case("reach %d" % d, s))
    for head, tail in (([1, 2], []), ([], [7, 9])):
        s = Stream(); s.stored(bytes(_rand(rng, 32768)))
        s.fixed(head + [(258, 32768)] * 127 + tail, final=True)
        c = _case("65536 bytes, last symbol %s" % ("two literals" if tail else "(258, 32768)"), s)
        assert len(c.expected) == 65536
        cases.append(c)
    return cases


def family_long_codes():
    """4: literal / length codes of 2 .. 15 bits (15 bits: a literal, a length symbol below 275, one at or above 275; 10 and 11 bits: either
    side of the device's index, 11 is the host's), distance codes of 1 .. 15 bits; every code used, the long ones some hundred times"""
    rng = np.random.default_rng(104)
    pool = [2, 2, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 15, 15, 15]
    dist_syms = [0, 2, 4, 7, 10, 13, 16, 19, 21, 22, 23, 24, 25, 26, 27, 28]
    cases = []
    for v in range(3):
        lits = _rand(rng, 9)
        while len(set(lits)) < 9:
            lits = _rand(rng, 9)
        low, high = (257, 265, 264)[v], (275, 276, 275)[v]
        fifteen = [lits[0], low, high, 256 if v == 0 else lits[1]]
        rest = [x for x in lits + [256, 257, 259, 264, 265, 274, 275, 276, 285] if x not in fifteen]
        rest = [rest[int(k)] for k in rng.permutation(len(rest))]
        rest.sort(key=lambda x: x < 274)  # (the long lengths that are drawn seldom, to keep the output small, take the short codes)
        assert len(rest) == 14
        lit_lens = [0] * 286
        for sym, l in zip(rest + fifteen, pool):
            lit_lens[sym] = l
        dist_lens = [0] * 30
        dl = list(range(1, 16)) + [15]
        for k in rng.permutation(16):
            dist_lens[dist_syms[int(k)]] = dl.pop()
        assert kraft(lit_lens) == 32768 and kraft(dist_lens) == 32768
        toks = []
        for sym in rest + fifteen:
            if sym == 256:
                continue
            cnt = 250 if lit_lens[sym] >= 11 else 100
            if sym >= 274 and lit_lens[sym] < 11:
                cnt = 40 if sym < 285 else 12
            if sym == 257:
                cnt = max(cnt, 1500)
            toks += [sym] * cnt
        toks = [toks[int(k)] for k in rng.permutation(len(toks))]
        # distance symbols: the long codes four times as often as the short ones
        dpool = [ds for ds in dist_syms for _ in range(4 if dist_lens[ds] >= 9 else 1)]
        out = []
        for t in toks:
            if t < 256:
                out.append(t); continue
            ln = LEN_BASE[t - 257] + int(rng.integers(0, 1 << LEN_EXTRA[t - 257]))
            ds = dpool[int(rng.integers(0, len(dpool)))]
            out.append((ln, DIST_BASE[ds] + int(rng.integers(0, 1 << DIST_EXTRA[ds]))))
        used = collections.Counter(dsym(t[1])[0] for t in out if type(t) is tuple)
        assert all(used[ds] >= (150 if dist_lens[ds] >= 9 else 1) for ds in dist_syms), used
        for header in ("plain", "rle"):
            s = Stream(); s.stored(bytes(_rand(rng, 26000)))
            s.dynamic(out, lit_lens, dist_lens, final=True, header=header)
            c = _case("long codes %d %s" % (v, header), s)
            assert len(c.expected) <= 65536, len(c.expected)
            cases.append(c)
    return cases


def family_literal_pairs():
    """5: literals of 2 .. 5 bits, so that every look-up of the device's table is a pair.  Behind one stored byte the pairs start at the odd
    positions: at SEG - 1, RING - 1 and out_len - 259 (one byte past the stop of the hand-written loop); without it at the even ones
    (they end on the stop).  j of the first 7 literals take 3 bits, the others 2: the 8 bit phases."""
    rng = np.random.default_rng(105)
    lit_lens = [0] * 257
    for sym, l in zip((65, 67, 71, 84, 78, 10, 48, 49, 50, 256), (2, 2, 3, 3, 4, 4, 5, 5, 5, 5)):
        lit_lens[sym] = l
    assert kraft(lit_lens) == 32768
    body = [(65, 67, 71, 84, 78, 10, 48, 49, 50)[k] for k in _rand(rng, 4696 - 8, 0, 9)]
    cases = []
    for odd in (1, 0):
        for j in range(8):
            s = Stream()
            if odd:
                s.stored(b"G")
            s.dynamic([71] * j + [65] * (7 - j) + body[:len(body) - (0 if odd else 1)], lit_lens, [0], final=True)
            c = _case("pairs at %s positions, phase %d" % ("odd" if odd else "even", j), s)
            assert len(c.expected) == (4696 if odd else 4694)
            cases.append(c)
    return cases


def _lens_286():
    return [8] * 226 + [9] * 60, [4] * 2 + [5] * 28  # complete codes with every symbol present


def family_headers():
    """6: block headers"""
    rng = np.random.default_rng(106)
    cases = []
    l286, d30 = _lens_286()
    assert kraft(l286) == 32768 and kraft(d30) == 32768

    def toks_all(n):
        t = _rand(rng, 400)
        for k in range(n):
            t.append((int(rng.integers(3, 259)), int(rng.integers(1, 400)))); t += _rand(rng, int(rng.integers(0, 4)))
        return t
    for header in ("plain", "rle", "widest"):
        s = Stream(); s.dynamic(toks_all(60), l286, d30, final=True, header=header)
        cases.append(_case("HLIT 286 HDIST 30 %s" % header, s))
    l257 = [8] * 255 + [9] * 2
    for header in ("plain", "rle"):
        s = Stream(); s.dynamic(_rand(rng, 500), l257, [0], final=True, header=header)
        cases.append(_case("HLIT 257 HDIST 1, no distance code, %s" % header, s))
    # the longest header behind a stored block: its start sweeps the window of compressed bytes (reloaded where fewer than 576 are left)
    for n in range(320, 901, 29):
        s = Stream(); s.stored(bytes(_rand(rng, n)))
        s.dynamic(toks_all(12), l286, d30, final=True, header="widest")
        cases.append(_case("widest header behind %d stored bytes" % n, s))
    # symbol 16 from the literal lengths into the distance lengths
    # 256 .. 259 four codes of 3 bits, 32 literals of 6 bits; eight distance codes of 3 bits: the run of 3s goes on across the boundary
    lit = [6] * 32 + [0] * 224 + [3] * 4; dst = [3] * 8
    assert kraft(lit) == 32768 and kraft(dst) == 32768
    r = rle_symbols(lit + dst)
    assert any(sym == 16 and a < 260 < a + k for sym, _, _, a, k in r), r
    s = Stream(); s.dynamic(_rand(rng, 50, 0, 32) + [(4, 7), (5, 3), 5, (3, 16)], lit, dst, final=True, header="rle")
    cases.append(_case("symbol 16 across the boundary between literal and distance lengths", s))
    # symbol 18 with a count of 138
    lit = [7] * 100 + [0] * 138 + [7] * 28; assert len(lit) == 266 and kraft(lit) == 32768
    r = rle_symbols(lit + [1, 1])
    assert (18, 127, 7, 100, 138) in r
    s = Stream(); s.dynamic(_rand(rng, 80, 0, 100) + [(3, 1), (9, 2)], lit, [1, 1], final=True, header="rle")
    cases.append(_case("symbol 18 with a count of 138", s))
    # HCLEN: with 4 only 16, 17, 18 and 0 have codes, so every length is 0 and the end-of-block code is missing: malformed.  5 adds the
    # length 8: the smallest valid header (256 codes of 8 bits)
    s = Stream(); s.dynamic([], [0] * 257, [0], final=True, hclen=4, cl_lens=[1] + [0] * 17 + [1], cl_syms=[(18, 127, 7), (18, 109, 7)], eob=False)
    cases.append(_case("HCLEN 4", s, valid=False))
    lit = [8] * 255 + [0, 8]
    s = Stream(); s.dynamic(_rand(rng, 300, 0, 255), lit, [0], final=True, hclen=5, cl_lens=[1] + [0] * 7 + [1] + [0] * 10)
    cases.append(_case("HCLEN 5", s))
    # one distance code of 1 bit, used (the incomplete set RFC 1951 allows)
    l258 = [8] * 254 + [9] * 4; assert kraft(l258) == 32768
    s = Stream(); s.dynamic(_rand(rng, 100, 0, 254) + [(3, 1), 3, (3, 1), 9, 9, (3, 1)], l258, [1], final=True)
    cases.append(_case("one distance code of 1 bit", s, tag="single_dist"))
    s = Stream(); s.dynamic(_rand(rng, 100, 0, 254) + [Raw("L", 257), Raw(None, 0, 1, 1)], l258, [1], final=True)
    cases.append(_case("the undefined bit of a one-code distance set", s, valid=False))
    # a single literal / length code: the end of block
    s = Stream(); s.stored(bytes(_rand(rng, 100))); s.dynamic([], [0] * 256 + [1], [0], final=True)
    cases.append(_case("only an end-of-block code", s, tag="single_litlen"))
    # malformed headers
    s = Stream(); s.dynamic([1, 2, 3], [7] * 257, [0], final=True)
    cases.append(_case("over-subscribed literal set", s, valid=False))
    s = Stream(); s.dynamic([1, 2, 3], l257, [0], final=True, cl_lens=[2] + [0] * 7 + [2, 2] + [0] * 9)
    cases.append(_case("incomplete code-length code", s, valid=False))
    s = Stream(); s.dynamic([1, 2, 3], l257, [0], final=True, header="rle", cl_syms=[(16, 0, 2)] + [(l, 0, 0) for l in l257[3:] + [0]])
    cases.append(_case("symbol 16 first", s, valid=False))
    s = Stream(); s.dynamic([1, 2, 3], l257, [0], final=True, header="rle", cl_syms=[(l, 0, 0) for l in l257] + [(18, 0, 7)])
    cases.append(_case("a repeat past HLIT + HDIST", s, valid=False))
    bad = [8] * 256 + [0, 0, 0]; assert kraft(bad) == 32768
    s = Stream(); s.dynamic([1, 2, 3], bad, [0], final=True, eob=False)
    cases.append(_case("no end-of-block code", s, valid=False))
    return cases


def family_block_structure():
    """7: block structure"""
    rng = np.random.default_rng(107)
    cases = []
    for where in ("first", "middle", "last", "everywhere"):
        s = Stream()
        if where in ("first", "everywhere"): s.stored(b"")
        s.fixed(_rand(rng, 300) + [(30, 100)])
        if where in ("middle", "everywhere"): s.stored(b""); s.stored(b"")
        s.fixed(_rand(rng, 10) + [(200, 320)], final=where in ("first", "middle"))
        if where in ("last", "everywhere"): s.stored(b"", final=True)
        cases.append(_case("empty stored blocks: %s" % where, s))
    s = Stream(); s.stored(b"", final=True)
    cases.append(_case("only an empty stored block", s))
    # zlib's own flushes
    data = bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 30000)]) + bytes(_rand(rng, 3000))
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    comp = b""
    for k, p in enumerate(range(0, len(data), 777)):
        comp += c.compress(data[p:p + 777]) + c.flush(zlib.Z_FULL_FLUSH if k % 3 == 2 else zlib.Z_SYNC_FLUSH)
    comp += c.flush()
    cases.append(Case("zlib stream flushed every 777 bytes", comp, data, len(data), None))
    # many tiny dynamic blocks, matches into earlier ones
    s, op = Stream(), 0
    for b in range(60):
        toks = []
        for _ in range(100):
            if op > 10 and rng.integers(0, 3) == 0:
                toks.append((int(rng.integers(3, 40)), int(rng.integers(1, min(op, 3000) + 1)))); op += toks[-1][0]
            else:
                toks.append(int(rng.integers(0, 256))); op += 1
        lit_used = {t for t in toks if type(t) is int} | {lsym(t[0])[0] for t in toks if type(t) is tuple} | {256, 0}
        dist_used = {dsym(t[1])[0] for t in toks if type(t) is tuple} | {0, 1}
        s.dynamic(toks, flat_lens(286, lit_used), flat_lens(30, dist_used), final=b == 59, header=("plain", "rle")[b & 1])
    cases.append(_case("60 dynamic blocks", s))
    # stored blocks from every bit phase: a fixed block of j 9-bit literals ends 10 + j bits behind a byte boundary
    spans = sorted({1} | {x for R in RINGS for x in (R // 2 - 1, R // 2, R // 2 + 1, 3 * (R // 2) + 7)})
    phases = collections.defaultdict(set)
    for j in range(8):
        s, prev = Stream(), 0
        for n in spans:
            toks = []
            if prev:  # into the stored block before: from its first byte, its last byte, and across its end
                ln = max(3, min(prev, 258))
                toks = [(ln, prev), (3, 1), (max(3, min(prev, 40)), min(prev, 70) + ln + 3)]
            s.fixed(toks + _rand(rng, j, 144, 256))
            phases[n].add(s.phase())
            s.stored(bytes(_rand(rng, n))); prev = n
        s.fixed([(100, 6151), (50, 50), 1], final=True)
        cases.append(_case("stored blocks of every span, %d 9-bit literals in front" % j, s))
    assert all(len(v) == 8 for v in phases.values()), phases
    return cases


def family_output_sizes():
    """8: output sizes around the gates of both decoders, and the same streams announced one byte shorter and longer"""
    rng = np.random.default_rng(108)
    sizes = sorted({0, 1, 2, 257, 258, 259, 260, 65279, 65280, 65535, 65536} | {x + k for R in RINGS for x in (R // 2, R) for k in (-1, 0, 1)})
    cases = []
    for n in sizes:
        for match in (False, True):
            if match and n < 4:
                continue  # (the shortest stream that ends in a match: one literal and a match of 3)
            s = Stream()
            if match:
                ln = min(258, n - 1)
                s.fixed(_rand(rng, n - ln) + [(ln, min(n - ln, 300))], final=True)
            else:
                s.fixed(_rand(rng, n), final=True)
            c = _case("%d bytes, %s" % (n, "ending in a match" if match else "literals"), s)
            assert len(c.expected) == n
            cases.append(c)
            for wrong in (n - 1, n + 1):
                if 0 <= wrong <= 65536:
                    cases.append(Case(c.name + ", announced as %d" % wrong, c.stream, None, wrong, None, True))
    return cases


def family_undefined():
    """9: undefined symbols and references before the start of the output"""
    rng = np.random.default_rng(109)
    cases = []
    for sym in (286, 287):
        s = Stream(); s.fixed(_rand(rng, 600) + [Raw("L", sym), Raw("D", 3)] + _rand(rng, 400), final=True)
        cases.append(_case("fixed-code literal/length symbol %d" % sym, s, valid=False))
    for sym in (30, 31):
        s = Stream(); s.fixed(_rand(rng, 600) + [Raw("L", 260), Raw("D", sym, 5, 13)] + _rand(rng, 400), final=True)
        cases.append(_case("fixed-code distance symbol %d" % sym, s, valid=False))
    l286, d30 = _lens_286()
    s = Stream(); s.dynamic([1, 2, 3], l286 + [9], d30, final=True)
    cases.append(_case("HLIT 287", s, valid=False))
    s = Stream(); s.dynamic([1, 2, 3], l286, d30 + [5], final=True)
    cases.append(_case("HDIST 31", s, valid=False))
    for op in (0, 1, 5000):
        s = Stream()
        ds, x, xb = dsym(op + 1)
        s.fixed(_rand(rng, op) + [Raw("L", 259), Raw("D", ds, x, xb)] + _rand(rng, 995), final=True)
        cases.append(_case("distance %d at %d" % (op + 1, op), s, valid=False))
    s = Stream(); s.fixed(_rand(rng, 500)); s.w.bits(1, 1); s.w.bits(3, 2); s.w.bits(0x5A5A5A, 24)
    cases.append(_case("BTYPE 3", s, valid=False))
    s = Stream(); s.fixed(_rand(rng, 500)); s.stored(bytes(_rand(rng, 500)), final=True, nlen=500 ^ 0xFFFE)
    cases.append(_case("stored LEN / NLEN mismatch", s, valid=False))
    s = Stream(); s.fixed(_rand(rng, 500)); s.stored(bytes(_rand(rng, 499)), final=True, length=500)
    cases.append(_case("stored LEN beyond the input", s, valid=False))
    return cases


FAMILIES = collections.OrderedDict([
    ("copy_geometry", family_copy_geometry), ("far_copy", family_far_copy), ("max_reach", family_max_reach), ("long_codes", family_long_codes),
    ("literal_pairs", family_literal_pairs), ("headers", family_headers), ("block_structure", family_block_structure),
    ("output_sizes", family_output_sizes), ("undefined", family_undefined)])
_cache = {}


def family(name):
    """the cases of one family, built once"""
    if name not in _cache:
        _cache[name] = FAMILIES[name]()
    return _cache[name]


def host_accepts(c):
    """the verdict the host decoder owes a case"""
    return c.expected is not None and c.tag is None


def dump(path):
    n = 0
    with open(path, "wb") as f:
        for name in FAMILIES:
            for c in family(name):
                f.write(struct.pack("<IIB", len(c.stream), c.n_out, int(host_accepts(c))) + c.stream)
                n += 1
    return n


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--dump":
        print("%d cases" % dump(sys.argv[2]))
    else:
        sys.exit(__doc__)
