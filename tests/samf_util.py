"""Handcrafted inputs for the SAM-field kernels' row-loop pre-pass (cigar_k.hip: samf_dp8_run; cigar_ag.h: SamfPre) and a plain Python
statement of which first cigar calls it may take.  samFields / samFieldsPaired take result records as INPUT, so an item is put exactly
where the kernel can go wrong: a read of chosen length cut at a chosen location of the golden genome, edited, oriented, wrapped in
clipped bases, with a result record that says where it lies.  Shared by tests/test_zz_gpu_samf_prepass.py and its emulator twin."""
import numpy as np

from snap_amd import abi

NOT_FOUND_LOCATION = 0xFFFFFFFF
SAMF_PRE_MAX_W = 7                                   # cigar_ag.h
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in (b"AT", b"TA", b"CG", b"GC", b"at", b"ta", b"cg", b"gc"):
    _COMP[_a] = _b


def revcomp(x):
    return _COMP[np.asarray(x, dtype=np.uint8)[::-1]]


def align16(x):
    return (x + 15) & ~15


def samf_pre_rows(RL):
    return RL + 16


def prepass_launched(RL, use_affine_gap=True, n=1):
    """launch_samf_dp8 (snapgpu.hip): the pre-pass runs for reads of up to 400 bases whose eight groups' LDS rows, four waves to a
    workgroup, stay within 64 KiB -- which holds up to RL = 240."""
    group = align16(RL) + align16(samf_pre_rows(RL)) + 6 * align16(RL)             # samf_dp8_group_bytes
    return bool(use_affine_gap) and n > 0 and RL <= 400 and 4 * 8 * group <= 64 * 1024


def kernel_rl(lengths):
    """The RL a host call hands its kernels: the longest unclipped read of the batch, 64 at least (check_sam_reads)."""
    return max(64, int(max(lengths))) if len(lengths) else 64


class Geometry:
    """What the predicate needs of an index (DevIndex: contig_begin, n_bases, chromosome_padding)."""
    def __init__(self, ix):
        self.begin = [int(b) for b in ix.contig_begin]
        self.n_bases = int(ix.n_bases)
        self.pad = int(ix.chromosome_padding)

    def contig_at(self, loc):                                        # Genome::getContigAtLocation
        c = -1
        for i, b in enumerate(self.begin):
            if b <= loc:
                c = i
        return c

    def contig_end(self, c):                                         # beginningLocation + length (the padding included)
        return self.n_bases if c == len(self.begin) - 1 else self.begin[c + 1]


def eligible(geo, RL, U, front_clip, data_len, res, use_affine_gap=True):
    """samf_dp8_run's `elig`, restated: is the read's FIRST affine-gap cigar call (sam_fields_single_item's attempt 0, cigar_ag_item's pass 0)
    a banded call of at most two vectors per segment, inside its contig, clear of the contig's end?  res: one RESULT_DTYPE record (or
    anything indexable by its field names)."""
    status, score, d, loc = int(res["status"]), int(res["score"]), int(res["direction"]), int(res["location"])
    add_f = int(res["clipping_for_read_adjustment"])
    cb, ca = int(res["bases_clipped_before"]), int(res["bases_clipped_after"])
    ag_branch = bool(use_affine_gap) and (int(res["used_affine_gap_scoring"]) != 0 or score > 0)
    front, dlen = front_clip + add_f, data_len - add_f
    bcb = (U - dlen - front) if d == 1 else front
    bcb += cb
    clipped = dlen - cb - ca
    if not (status != abi.NOT_FOUND and ag_branch and 0 <= loc < geo.n_bases and 0 <= score <= SAMF_PRE_MAX_W and U <= RL and
            clipped >= 3 * (2 * score + 1) and bcb >= 0 and bcb + clipped <= U and dlen >= 0):
        return False
    c = geo.contig_at(loc)
    if c < 0:
        return False
    cend = geo.contig_end(c)
    return loc + dlen <= cend and loc + clipped <= cend - geo.pad and cend > loc + clipped


class Item:
    """One read and its result record.  bases / quals: the read as the FASTQ has it (U bytes); pattern / pattern_quals: the oriented,
    clipped part the cigar call sees, at `loc`; bcb / bca: the oriented read's bases before / after it."""
    __slots__ = ("cls", "tag", "bases", "quals", "front_clip", "data_len", "res", "pattern", "pattern_quals", "bcb", "bca", "loc", "k", "want")

    @property
    def U(self):
        return int(self.bases.size)


def make_result(status=abi.SINGLE_HIT, direction=0, location=NOT_FOUND_LOCATION, score=-1, used_ag=0, mapq=0, cb=0, ca=0):
    r = np.zeros(1, dtype=abi.RESULT_DTYPE)[0]
    r["status"], r["direction"], r["location"], r["orig_location"] = status, direction, location, location
    r["score"], r["score_prior_to_clipping"], r["mapq"] = score, score, mapq
    r["used_affine_gap_scoring"], r["bases_clipped_before"], r["bases_clipped_after"] = used_ag, cb, ca
    return r


def cut_and_edit(G, rng, p, n, edits):
    """n bases: the genome from location p on with `edits` applied, each ("S", offset) -- another base --, ("N", offset), ("I", offset, count)
    or ("D", offset, count), offsets counted in the unedited text; the later an edit lies the earlier it is applied."""
    r = [int(x) for x in G[p:p + n + 64]]
    for e in sorted(edits, key=lambda e: -e[1]):
        o = e[1]
        if e[0] == "S":
            r[o] = int(rng.choice([b for b in ACGT if b != r[o]]))
        elif e[0] == "N":
            r[o] = ord("N")
        elif e[0] == "I":
            r[o:o] = [int(b) for b in rng.choice(ACGT, size=e[2])]
        else:
            del r[o:o + e[2]]
    assert len(r) >= n
    return np.array(r[:n], dtype=np.uint8)


def make_item(G, rng, cls, p, n, k, edits=(), rc=False, used_ag=1, cb=0, ca=0, before=0, after=0, loc=None, tag="", want=None, mapq=None):
    """A read whose oriented form is [before junk][cb junk][n bases cut at p and edited][ca junk][after junk]: `before` / `after` are what
    Read::clip took off (front_clip / data_len), cb / ca the aligner's soft clipping (bases_clipped_before / bases_clipped_after).
    want: True / False where the class means the item to be taken / not taken by the pre-pass."""
    it = Item()
    core = cut_and_edit(G, rng, p, n, edits)
    junk = lambda m: rng.choice(ACGT, size=m).astype(np.uint8)
    oriented = np.concatenate([junk(before), junk(cb), core, junk(ca), junk(after)])
    U = oriented.size
    oq = rng.integers(35, 74, size=U).astype(np.uint8)
    it.cls, it.tag, it.k, it.want = cls, tag, k, want
    it.loc = p if loc is None else loc
    it.pattern, it.pattern_quals = core, oq[before + cb:before + cb + n].copy()
    it.bcb, it.bca = before + cb, ca + after
    it.bases, it.quals = (revcomp(oriented), oq[::-1].copy()) if rc else (oriented, oq)
    it.front_clip = after if rc else before
    it.data_len = cb + n + ca
    it.res = make_result(direction=1 if rc else 0, location=it.loc, score=k, used_ag=used_ag, cb=cb, ca=ca,
                         mapq=int(rng.integers(0, 71)) if mapq is None else mapq)
    return it


def unmapped_item(rng, U, cls="unmapped"):
    it = Item()
    it.cls, it.tag, it.k, it.want, it.loc = cls, "NotFound", -1, False, -1
    it.bases = rng.choice(ACGT, size=U).astype(np.uint8); it.quals = rng.integers(35, 74, size=U).astype(np.uint8)
    it.front_clip, it.data_len, it.bcb, it.bca = 0, U, 0, 0
    it.pattern, it.pattern_quals = it.bases, it.quals
    it.res = make_result(status=abi.NOT_FOUND)
    return it


class Maker:
    """The item classes for a kernel RL (= the longest read of every batch made from them)."""
    def __init__(self, ix, seed=2024):
        self.ix, self.geo = ix, Geometry(ix)
        self.G = ix.genome_padded[(ix.genome_padded.size - ix.n_bases) // 2:]            # (location 0 on, the padding behind the genome included)
        self.begin = self.geo.begin
        self.real_end = [self.geo.contig_end(c) - self.geo.pad for c in range(len(self.begin))]
        self.seed = seed

    def clean(self, rng, n, contig=0):
        """a location in the contig's interior whose next n + 200 bases hold no N"""
        while True:
            p = int(rng.integers(self.begin[contig] + 50, self.real_end[contig] - n - 250))
            if (self.G[p:p + n + 200] != ord("N")).all():
                return p

    def with_n(self, rng, n, contig=0):
        """a location with an N of the reference 10 .. n - 10 bases on"""
        where = np.flatnonzero(self.G[self.begin[contig]:self.real_end[contig] - 300] == ord("N")) + self.begin[contig]
        where = where[where > self.begin[contig] + n]
        return int(rng.choice(where)) - int(rng.integers(10, n - 10))

    def classes(self, RL):
        """{class: [Item]} -- every item at most RL bases long"""
        rng = np.random.default_rng(self.seed + RL)
        G, mk = self.G, lambda *a, **kw: make_item(self.G, rng, *a, **kw)
        out = {}
        # ---- band shapes: k = 0 .. 8; substitutions only, one insertion, one deletion, an indel run of k, edits at both ends
        L = out["band"] = []
        n = RL - 3
        for k in range(9):
            want = k <= SAMF_PRE_MAX_W
            spread = [("S", o) for o in np.linspace(1, n - 2, k).astype(int)] if k else []
            ends = [("S", o) for o in ([0, 1, 2, n - 3, n - 2, n - 1] + list(range(10, 10 + 2 * k, 2)))[:k]]
            variants = [("subs", spread), ("ends", ends)]
            if k:
                variants += [("ins1", [("I", n // 2, 1)] + spread[:k - 1]), ("del1", [("D", n // 2, 1)] + spread[:k - 1]),
                             ("insrun", [("I", n // 3, k)]), ("delrun", [("D", n // 3, k)]),
                             ("ins_at_end", [("S", 2)] * (k > 1) + [("I", n - 8, k - (k > 1))]), ("del_at_end", [("S", 1)] * (k > 1) + [("D", n - 8, k - (k > 1))])]
            for j, (tag, ed) in enumerate(variants):
                L.append(mk("band", self.clean(rng, n), n, k, ed, rc=bool((j + k) & 1), tag="k%d_%s" % (k, tag), want=want))
        L.append(mk("band", self.clean(rng, n), n, 0, rc=True, used_ag=1, tag="k0_exact_rc", want=True))
        for rc in (False, True):                                           # score 0 without affine-gap scoring: the Landau-Vishkin writer
            L.append(mk("band", self.clean(rng, n), n, 0, rc=rc, used_ag=0, tag="k0_lv", want=False))
        # ---- the shortest pattern the banded call accepts, one less, one more
        L = out["shortest"] = []
        for k in range(8):
            for j, n in enumerate((3 * (2 * k + 1) - 1, 3 * (2 * k + 1), 3 * (2 * k + 1) + 1)):
                if n > RL:
                    continue
                ed = [("S", o) for o in (n // 3, 2 * n // 3)[:min(k, 2)]]
                L.append(mk("shortest", self.clean(rng, n), n, k, ed, rc=bool((j + k) & 1), tag="k%d_n%d" % (k, n), want=n >= 3 * (2 * k + 1)))
        # ---- the row cap: U = RL - 17 .. RL with nothing clipped, an indel of k bases near the read's end
        L = out["rowcap"] = []
        for j, U in enumerate(range(RL - 17, RL + 1)):
            special = U == RL or (U - 1) % 8 == 0
            for k in ((3, 4, 7) if special else ((3, 4, 7)[j % 3],)):
                if U < 3 * (2 * k + 1):
                    continue
                for kind in ("DI" if special else "DI"[j & 1]):
                    L.append(mk("rowcap", self.clean(rng, U), U, k, [(kind, U - 8, k)], rc=bool((j + k + (kind == "I")) & 1), tag="U%d_k%d_%s" % (U, k, kind), want=True))
        # ---- contig geometry
        L = out["contig"] = []
        n = min(RL - 2, 100)
        last = len(self.begin) - 1
        for c in range(len(self.begin)):
            e, cend = self.real_end[c], self.geo.contig_end(c)
            for rc in (False, True):
                L.append(mk("contig", e - n, n, 1, [("S", n // 2)], rc=rc, tag="c%d_ends_on_last_base" % c, want=True))
                L.append(mk("contig", e - n + 1, n, 1, [("S", n // 2)], rc=rc, tag="c%d_one_past" % c, want=False))
                L.append(mk("contig", self.begin[c], n, 1, [("S", n // 2)], rc=rc, tag="c%d_first_base" % c, want=True))
            L.append(mk("contig", e - n - 3, n, 3, [("D", n - 8, 3)], tag="c%d_deletion_runs_to_last_base" % c, want=True))
            L.append(mk("contig", cend - n - 2, n, 1, ca=2, tag="c%d_data_ends_at_cend" % c, want=False))        # loc + data_len == cend, in the padding
            if c != last:                                                                                       # loc + data_len > cend: `extra` (not past the genome's
                L.append(mk("contig", cend - n, n, 1, ca=2, rc=True, tag="c%d_data_past_cend" % c, want=False)) #  end, which no aligner reports and the entry points do not expect)
                for rc in (False, True):                                                                        # ... with bases left beyond `extra`: 5 in the padding, the rest
                    L.append(mk("contig", cend - 5, n, 2, [("S", n // 2)], rc=rc, tag="c%d_hangs_into_next" % c, want=False))   #  on the next contig
            L.append(mk("contig", self.clean(rng, n, c), n, 2, [("S", 5), ("S", n - 6)], rc=bool(c & 1), tag="c%d_interior" % c, want=True))
        L.append(mk("contig", self.begin[0] - n // 2, n, 1, tag="before_first_contig", want=False))
        # ---- a leading indel: the first attempt returns add_front_clipping != 0, the record comes from a retry
        L = out["leading"] = []
        n = RL - 4
        for j, (tag, ed, shift) in enumerate([("ins1_at0", [("I", 0, 1)], 0), ("ins2_at0", [("I", 0, 2)], 0), ("ins1_at1", [("I", 1, 1)], 0), ("ins2_at1", [("I", 1, 2)], 0),
                                              ("del1_at0", [], 1), ("del2_at0", [], 2), ("del3_at0", [], 3), ("del2_at1", [("D", 1, 2)], 0)]):
            for rc in (False, True):
                p = self.clean(rng, n)
                L.append(mk("leading", p + shift, n, 3, ed, rc=rc, loc=p, tag=tag, want=True))
        # ---- N in the read, N in the reference window: the profile's -1
        L = out["n"] = []
        n = RL - 5
        for j in range(3):
            L.append(mk("n", self.clean(rng, n), n, 3, [("N", 4 + j), ("N", n // 2), ("N", n - 2 - j)], rc=bool(j & 1), tag="read_N", want=True))
            L.append(mk("n", self.with_n(rng, n, j % 2), n, 4, [("S", 7)], rc=bool(j & 1), tag="ref_N", want=True))
            L.append(mk("n", self.with_n(rng, n, j % 2), n, 5, [("N", n // 3), ("D", n - 9, 2)], rc=not (j & 1), tag="both_N", want=True))
        for j, c in enumerate((0, len(self.begin) - 1)):                    # the rows past the pattern read the padding's n: the read ends 2 bases before
            m = min(n, 90)                                                   #  the contig's last real one, 4 of them deleted 10 bases before
            L.append(mk("n", self.real_end[c] - m - 6, m, 4, [("D", m - 10, 4)], rc=bool(j), tag="c%d_window_in_padding" % c, want=True))
        # ---- unmapped: NotFound results between the others, of every length class
        L = out["unmapped"] = []
        for j, U in enumerate((RL - 1, 21, RL // 2, 1)):
            L.append(unmapped_item(rng, U))
            m = RL - 2 - j
            L.append(mk("unmapped", self.clean(rng, m), m, 2 * j, [("S", o) for o in range(3, 3 + 4 * j, 2)], rc=bool(j & 1), tag="mapped_between", want=True))
        L.append(unmapped_item(rng, RL - 3))
        # ---- clip windows: Read::clip in front and behind, the aligner's soft clipping, both directions
        L = out["clip"] = []
        for j, (b, a, cb, ca) in enumerate([(3, 0, 0, 0), (0, 4, 0, 0), (0, 0, 5, 0), (0, 0, 0, 6), (2, 3, 0, 0), (0, 0, 4, 1), (1, 2, 3, 4), (7, 0, 0, 5), (0, 9, 6, 0)]):
            for rc in (False, True):
                n = RL - (b + a + cb + ca) - (j & 1)
                k = (1, 5, 2, 7)[j % 4]
                ed = [("S", 3), ("I" if j & 2 else "D", n // 2, max(1, k - 2))] + ([("S", n - 4)] if k > 2 else [])
                L.append(mk("clip", self.clean(rng, n), n, k, ed[:k], rc=rc, cb=cb, ca=ca, before=b, after=a, tag="b%d_a%d_cb%d_ca%d" % (b, a, cb, ca), want=True))
        for items in out.values():
            assert all(it.U <= RL for it in items)
        return out

    def pin(self, RL, seed=0):
        """A NotFound read of RL bases: wherever it stands in a batch, the batch's kernels run with this RL."""
        return unmapped_item(np.random.default_rng(self.seed + 7 * RL + seed), RL)


def pack(items):
    """The arrays samFields takes."""
    lens = [it.U for it in items]
    return dict(bases=np.concatenate([it.bases for it in items]), quals=np.concatenate([it.quals for it in items]),
                offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64),
                front_clip=np.array([it.front_clip for it in items], np.int32), data_len=np.array([it.data_len for it in items], np.int32),
                results=np.array([it.res for it in items], dtype=abi.RESULT_DTYPE))


def predicate(geo, items, use_affine_gap=True):
    """Per item: would the pre-pass kernel take it, in a batch of exactly these items?"""
    RL = kernel_rl([it.U for it in items])
    return np.array([eligible(geo, RL, it.U, it.front_clip, it.data_len, it.res, use_affine_gap) for it in items], dtype=bool)


def expected_valid(geo, items, use_affine_gap=True):
    RL = kernel_rl([it.U for it in items])
    return int(predicate(geo, items, use_affine_gap).sum()) if prepass_launched(RL, use_affine_gap, len(items)) else 0


def pair_up(geo, items):
    """Mates for samFieldsPaired: the mapped items that lie inside their contig (extra == 0) two by two, both on one contig, aligned_as_pair
    set.  Returns (mates in order, results)."""
    by_contig = {}
    for it in items:
        c = geo.contig_at(it.loc)
        if int(it.res["status"]) == abi.NOT_FOUND or c < 0:
            continue
        # A mate that hangs over its contig's end is formatted at `extra` = the next contig's beginning - loc.  Kept, unless that leaves a pattern
        # of NO bases (the read wholly in the padding): computeGlobalScore divides by its vector count, 0 then -- agc_full as the reference.
        extra = geo.contig_end(c) - it.loc if it.loc + it.data_len > geo.contig_end(c) else 0
        if it.pattern.size - extra > 0:
            by_contig.setdefault(c, []).append(it)
    mates = []
    for c in sorted(by_contig):
        group = by_contig[c]
        mates += group[:len(group) & ~1]
    res = np.zeros(len(mates) // 2, dtype=abi.PAIRED_RESULT_DTYPE)
    for i, it in enumerate(mates):
        for f in abi.RESULT_DTYPE.names:
            if f in abi.PAIRED_RESULT_DTYPE.names and res[f].ndim == 2:
                res[f][i >> 1, i & 1] = it.res[f]
    res["aligned_as_pair"] = 1
    return mates, res
