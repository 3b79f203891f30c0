"""Host-side mirror of the steps of analyze_tr that sit in FRONT of the GPU path: catalog + reference + BAM -> Locus + clipped reads.

Reference (PacificBiosciences/trgt v3.0.0):
  Locus (flanks from the genome)      src/trgt/locus.rs:13-23, 168-190        -> read_catalog
  extract_reads                       src/trgt/workflows/tr.rs:262-361        -> extract_reads
  HiFiRead::clip_to_region            src/trgt/reads/clip_region.rs:19-184    -> clip_to_region
  clip_reads                          src/trgt/workflows/tr.rs:186-196        -> clip_reads

Plain Python over zlib (BGZF is a multi-member gzip stream): the reference does this through htslib, which is I/O plumbing outside
the hot path; nothing here touches the GPU.  Not mirrored: methylation tags (MM/ML), SNV mismatch offsets, HP tags -- the locus path
behind them (get_meth, genotype_flank) is out of scope, so reads carry bases and the rq tag only.

Reservoir sampling of loci deeper than 3 x max_depth (tr.rs:311-335) draws from rand 0.9's StdRng::seed_from_u64(42).  Its stream is
restated below in plain Python integers from the published algorithms (ChaCha: Bernstein 2008 / RFC 8439 2.1-2.3; PCG32 XSH-RR: O'Neill
2014; Canon's range sampling as rand 0.9 documents it), on its own and not from trgt_amd/csrc/ingest.hip, so that it can stand as a
third party between the host's StdRng and the kernel's DevRng.  What that gives: chacha_block is PINNED by published vectors
(tests/golden/chacha_vectors.json); the seed expansion, the order the words are read in and the range sampling agree across three
separately written implementations -- second draw, 64-bit ranges and the straddling next_u64 included -- but are not pinned by any
value that rand itself produced (none can be made where this was written).
"""
import gzip
import struct
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

REF_CONSUMING = {0, 2, 3, 7, 8}  # M D N = X
QRY_CONSUMING = {0, 1, 4, 7, 8}  # M I S = X
SPLITTABLE = {0, 2, 3, 7, 8}
_SEQ_CODE = "=ACMGRSVTWYHKDBN"


@dataclass
class Locus:  # locus.rs:13-23
    id: str
    contig: str
    start: int
    end: int
    left_flank: bytes
    tr: bytes
    right_flank: bytes
    motifs: List[str]
    struc: str
    ploidy: int = 2
    genotyper: str = "size"


@dataclass
class BamRecord:
    name: str
    contig: Optional[str]
    pos: int
    flag: int
    cigar: List[Tuple[int, int]]  # (op code, length)
    seq: str
    rq: Optional[float]


def read_fasta(path) -> Dict[str, str]:
    seqs, name = {}, None
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                name = line[1:].split()[0]
                seqs[name] = []
            elif name is not None:
                seqs[name].append(line)
    return {k: "".join(v) for k, v in seqs.items()}


def read_catalog(bed_path, genome: Dict[str, str], flank_len=250, genotyper="size") -> List[Locus]:
    """repeat catalog (BED: contig, start, end, ID=..;MOTIFS=..;STRUC=..) -> loci with upper-cased flanks (locus.rs:168-190)"""
    loci = []
    for line in open(bed_path):
        if not line.strip():
            continue
        contig, start, end, info = line.split()[:4]
        start, end = int(start), int(end)
        f = dict(x.split("=", 1) for x in info.split(";"))
        g = genome[contig]
        if start < flank_len or end + flank_len > len(g):
            raise ValueError("locus %s: flanks leave the contig" % f["ID"])
        loci.append(Locus(f["ID"], contig, start, end, g[start - flank_len:start].upper().encode(), g[start:end].upper().encode(),
                          g[end:end + flank_len].upper().encode(), f["MOTIFS"].split(","), f["STRUC"], 2, genotyper))
    return loci


def _rq_tag(buf):
    i = 0
    size = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
    while i < len(buf):
        tag, ty = buf[i:i + 2], chr(buf[i + 2])
        i += 3
        if ty in size:
            if tag == b"rq" and ty == "f":
                return struct.unpack_from("<f", buf, i)[0]
            i += size[ty]
        elif ty in "ZH":
            i = buf.index(b"\0", i) + 1
        elif ty == "B":
            sub, n = chr(buf[i]), struct.unpack_from("<I", buf, i + 1)[0]
            i += 5 + n * size[sub]
        else:
            raise ValueError("bad BAM tag type " + ty)
    return None


def read_bam(path) -> List[BamRecord]:
    data = gzip.open(path, "rb").read()
    if data[:4] != b"BAM\1":
        raise ValueError("not a BAM file")
    p = 8 + struct.unpack_from("<i", data, 4)[0]
    n_ref = struct.unpack_from("<i", data, p)[0]
    p += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", data, p)[0]
        refs.append(data[p + 4:p + 4 + l_name - 1].decode())
        p += 8 + l_name
    out = []
    while p < len(data):
        bs = struct.unpack_from("<i", data, p)[0]
        rec = data[p + 4:p + 4 + bs]
        p += 4 + bs
        ref_id, pos, l_rn, _mapq, _bin, n_cig, flag, l_seq, _nr, _np, _tl = struct.unpack_from("<iiBBHHHiiii", rec, 0)
        q = 32
        name = rec[q:q + l_rn - 1].decode()
        q += l_rn
        cigar = [(v & 0xF, v >> 4) for v in struct.unpack_from("<%dI" % n_cig, rec, q)]
        q += 4 * n_cig
        packed = rec[q:q + (l_seq + 1) // 2]
        q += (l_seq + 1) // 2 + l_seq
        seq = "".join(_SEQ_CODE[(packed[i >> 1] >> (4 if i % 2 == 0 else 0)) & 0xF] for i in range(l_seq))
        out.append(BamRecord(name, refs[ref_id] if ref_id >= 0 else None, pos, flag, cigar, seq, _rq_tag(rec[q:])))
    return out


# ---- rand 0.9: StdRng::seed_from_u64(seed).random_range(0..n), from the published algorithms --------------------------------------------
_M32, _M64 = (1 << 32) - 1, (1 << 64) - 1
_CONSTANTS = struct.unpack("<4I", b"expand 32-byte k")
_COLUMNS = ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15))
_DIAGONALS = ((0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14))


def _quarter_round(s, a, b, c, d):
    """RFC 8439 2.1: a += b; d ^= a; d <<<= 16;  c += d; b ^= c; b <<<= 12;  a += b; d ^= a; d <<<= 8;  c += d; b ^= c; b <<<= 7"""
    for x, y, z, left in ((a, b, d, 16), (c, d, b, 12), (a, b, d, 8), (c, d, b, 7)):
        s[x] = (s[x] + s[y]) & _M32
        v = s[z] ^ s[x]
        s[z] = ((v << left) | (v >> (32 - left))) & _M32


def chacha_block(key_words, counter64, stream64, rounds):
    """One 16-word ChaCha block.  State: the four constants, the eight key words, then 128 bits that Bernstein's ChaCha (and rand_chacha)
    read as a 64-bit block counter (words 12-13) and a 64-bit stream id (14-15), RFC 8439 as a 32-bit counter and a 96-bit nonce.
    `rounds` / 2 double rounds (a column round, a diagonal round), then the input state is added word by word."""
    assert len(key_words) == 8 and rounds % 2 == 0
    start = list(_CONSTANTS) + [k & _M32 for k in key_words] + [counter64 & _M32, (counter64 >> 32) & _M32, stream64 & _M32, (stream64 >> 32) & _M32]
    s = list(start)
    for _ in range(rounds // 2):
        for q in _COLUMNS:
            _quarter_round(s, *q)
        for q in _DIAGONALS:
            _quarter_round(s, *q)
    return [(x + y) & _M32 for x, y in zip(s, start)]


def seed_from_u64(state):
    """rand_core's SeedableRng::seed_from_u64 for a 32-byte seed: eight outputs of PCG32 (XSH-RR 64/32; the state advances BEFORE each
    output), each written little-endian -- read back as little-endian key words they are the outputs themselves"""
    words = []
    for _ in range(8):
        state = (state * 6364136223846793005 + 11634580027462260723) & _M64
        xorshifted = (((state >> 18) ^ state) >> 27) & _M32
        rot = state >> 59
        words.append(((xorshifted >> rot) | (xorshifted << (32 - rot))) & _M32 if rot else xorshifted)
    return words


class StdRng:
    """rand 0.9's StdRng: ChaCha with 12 rounds behind rand_core's BlockRng -- a buffer of 64 words (four consecutive blocks per refill),
    read in order; it starts empty.  The counters (`refills`, `u64_cases`, `second_draws`, `carries`) let a test assert that its inputs
    reached a branch."""

    def __init__(self, seed=42, key=None, rounds=12, counter=0, stream=0):
        self.key = list(key) if key is not None else seed_from_u64(seed)
        self.rounds, self.counter, self.stream = rounds, counter, stream
        self.results, self.index = [0] * 64, 64
        self.refills, self.u64_cases, self.second_draws, self.carries = 0, [0, 0, 0], 0, 0

    def _generate(self):
        self.results = [w for b in range(4) for w in chacha_block(self.key, (self.counter + b) & _M64, self.stream, self.rounds)]
        self.counter = (self.counter + 4) & _M64
        self.refills += 1

    def next_u32(self):
        if self.index >= 64:
            self._generate()
            self.index = 0
        self.index += 1
        return self.results[self.index - 1]

    def next_u64(self):
        """BlockRng::next_u64: two words, the first one the low half -- [0] both still in the buffer; [1] the buffer is used up: refill,
        words 0 and 1; [2] one word left: it is the low half, the high half is word 0 of the refilled buffer, and reading goes on at 1"""
        i = self.index
        if i < 63:
            self.u64_cases[0] += 1
            self.index = i + 2
            return (self.results[i + 1] << 32) | self.results[i]
        if i >= 64:
            self.u64_cases[1] += 1
            self._generate()
            self.index = 2
            return (self.results[1] << 32) | self.results[0]
        self.u64_cases[2] += 1
        low = self.results[63]
        self._generate()
        self.index = 1
        return (self.results[0] << 32) | low

    def random_range(self, n):
        """rng.random_range(0..n) for usize on a 64-bit target (n >= 1).  The half-open range is sampled as the inclusive 0 ..= n - 1;
        when that upper bound fits in u32 the sample type is u32, else u64.  Canon's method: one widening multiplication of a random
        word by the span; only if the low half of the product exceeds -span (in the sample type) a second word is drawn, and the high half
        of ITS product is added to that low half -- a carry out of the addition bumps the result.  A span that wraps to 0 is the whole
        type: the random word itself."""
        high = n - 1
        bits, draw = (32, self.next_u32) if high <= _M32 else (64, self.next_u64)
        mask = (1 << bits) - 1
        span = (high + 1) & mask
        if span == 0:
            return draw()
        product = draw() * span
        result, low = product >> bits, product & mask
        if low > ((-span) & mask):
            self.second_draws += 1
            if low + ((draw() * span) >> bits) > mask:
                self.carries += 1
                result += 1
        return result


def extract_reads_seen(locus: Locus, records: List[BamRecord], flank_len=250, min_read_qual=0.98, max_depth=250):
    """tr.rs:262-361: records overlapping region +- flank_len, in file order.  The first 3 * max_depth that pass the filters fill the
    reservoir; every further one draws j = random_range(0..reads so far) from StdRng::seed_from_u64(42) and replaces slot j when
    j < 3 * max_depth (secondary / supplementary / low-rq records draw nothing).  A record with the unmapped bit set that the fetch returns
    counts like any other (clip_to_region drops it later).  Returns (records in slot order, number dropped for quality, reads seen)."""
    lo, hi = max(0, locus.start - flank_len), locus.end + flank_len
    reservoir = 3 * max_depth
    reads, n_filt, n_reads, rng = [], 0, 0, None
    for r in records:
        if r.contig != locus.contig:
            continue
        ref_end = r.pos + sum(n for c, n in r.cigar if c in REF_CONSUMING)
        if ref_end <= lo or hi <= r.pos:
            continue
        if r.flag & (0x100 | 0x800):  # secondary / supplementary
            continue
        if (r.rq if r.rq is not None else 1.0) < min_read_qual:
            n_filt += 1
            continue
        if n_reads < reservoir:
            reads.append(r)
        else:
            if rng is None:
                rng = StdRng(42)
            j = rng.random_range(n_reads)
            if j < reservoir:
                reads[j] = r
        n_reads += 1
    return reads, n_filt, n_reads


def extract_reads(locus: Locus, records: List[BamRecord], flank_len=250, min_read_qual=0.98, max_depth=250):
    """extract_reads_seen without the count: (records, number dropped for quality)"""
    return extract_reads_seen(locus, records, flank_len, min_read_qual, max_depth)[:2]


def clip_cigar(ref_pos0, ops, region):
    """clip_region.rs:108-184: (ref_start, query_start, ops) of the part of the alignment inside region, or None"""
    rs, re_ = region
    rlen = lambda o: o[1] if o[0] in REF_CONSUMING else 0
    qlen = lambda o: o[1] if o[0] in QRY_CONSUMING else 0
    if ref_pos0 + sum(rlen(o) for o in ops) <= rs or re_ <= ref_pos0:
        return None
    ref_pos, query_pos, i, out = ref_pos0, 0, 0, []
    while i < len(ops) and ref_pos + rlen(ops[i]) <= rs:
        ref_pos += rlen(ops[i]); query_pos += qlen(ops[i]); i += 1
    c_ref, c_qry = ref_pos, query_pos
    if ref_pos < rs:
        outside, op = rs - ref_pos, ops[i]
        assert op[0] in SPLITTABLE
        out.append((op[0], rlen(op) - outside if ref_pos + rlen(op) <= re_ else re_ - rs))
        c_ref += outside
        if qlen(out[-1]) != 0:
            c_qry += outside
        ref_pos += rlen(op); query_pos += qlen(op); i += 1
    while i < len(ops) and ref_pos + rlen(ops[i]) <= re_:
        out.append(ops[i]); ref_pos += rlen(ops[i]); query_pos += qlen(ops[i]); i += 1
    if i < len(ops) and ref_pos < re_:
        assert ops[i][0] in SPLITTABLE
        out.append((ops[i][0], re_ - ref_pos))
    return c_ref, c_qry, out


def clip_to_region(rec: BamRecord, region) -> Optional[bytes]:
    """HiFiRead::clip_to_region (clip_region.rs:19-76), bases only (a record with the unmapped bit carries no alignment: no read)"""
    if rec.flag & 0x4:
        return None
    r = clip_cigar(rec.pos, rec.cigar, region)
    if r is None:
        return None
    _, q0, ops = r
    n = sum(o[1] for o in ops if o[0] in QRY_CONSUMING)
    return rec.seq[q0:q0 + n].encode()


def clip_reads(locus: Locus, radius: int, reads: List[BamRecord]):
    """tr.rs:186-196; returns (clipped bases, rq) of the reads that overlap region +- radius"""
    region = (locus.start - radius, locus.end + radius)
    out = []
    for r in reads:
        s = clip_to_region(r, region)
        if s is not None:
            out.append((s, r.rq))
    return out


def locus_inputs(locus: Locus, records: List[BamRecord], flank_len=250, min_read_qual=0.98, max_depth=250):
    """Everything analyze_tr does before get_spanning_reads (tr.rs:29-35): the dict trgt_amd.locus.pack takes."""
    reads, _ = extract_reads(locus, records, flank_len, min_read_qual, max_depth)
    clipped = clip_reads(locus, 2 * flank_len, reads)
    return dict(left_flank=locus.left_flank, right_flank=locus.right_flank, tr=locus.tr, motifs=[m.encode() for m in locus.motifs],
                ploidy=locus.ploidy, genotyper=locus.genotyper, reads=[s for s, _ in clipped], read_qual=[q for _, q in clipped])
