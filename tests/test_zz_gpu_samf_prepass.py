"""The eight-reads-per-wave row-loop pre-pass of the SAM-field kernels (cigar_k.hip: samf_dp8_run -> k_samf_dp8, k_samf_dp8_rec,
k_samf_dp8_paired; cigar_ag.h: SamfPre, agc_from_pre) at its edges, on handcrafted items (tests/samf_util.py): band widths 0 .. 8, the
shortest pattern the banded call accepts, reads within 17 bases of the kernels' RL (the row cap RL + 16), contig ends and beginnings, the
ALT contig, leading indels, N, every clip window, unmapped reads in between; in batches of 1 .. 69 items, waves with one eligible group,
with none, with one- and two-vector groups side by side, and a seeded random order.

What is checked, bit for bit:
  1. snapgpu_debug_samf_pre_valid == the count of samf_util.eligible (a plain Python statement of the kernel's predicate) after every call,
     0 with SNAPGPU_SAMF_DP8=0 and on a context without affine gap;
  2. every output with the pre-pass == every output without it (a child process with SNAPGPU_SAMF_DP8=0: agc_banded_par runs instead);
  3. the records of the eligible items == the compiled reference's computeCigar on the oriented, clipped pattern (where oracle/_ref is built);
  4. the same for the mates of samFieldsPaired and the records of alignSamRecords;
  5. cigar_properties (tests/test_zz_gpu_cigar.py) on every mapped record.
The kernels' RL is the longest read of a batch (64 at least), so every batch holds a read of exactly RL bases.  The pre-pass is launched up to
RL = 240 (its LDS rows for four waves stay within 64 KiB); the batches at RL = 400 pin that nothing is taken there and nothing changes.
The row-cap class runs at RL = 145 too: a read of 145 = 9 * 16 + 1 bases with k = 7 stays active to row 166, the cap RL + 16 ends it at row 160.
A mate that hangs over its contig's end goes into the paired batch unless nothing of it is left beyond `extra` (samf_util.pair_up).

The check_* functions are shared with the emulator twin (tests/test_emu_samf_prepass.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from snap_amd import abi
from tests import samf_util as su
from tests import util
from tests.test_zz_gpu_cigar import cigar_properties

KEYS = ("flag", "contig", "pos", "mapq", "n_ops", "ops", "nm", "stale")
PAIRED_KEYS = KEYS + ("rnext", "pnext", "tlen", "first_written")
REC_KEYS = KEYS + ("rec_begin", "rec_read", "rec_kind")
BATCH_SIZES = (1, 7, 8, 9, 31, 32, 33, 69)
ELIGIBLE_CLASSES = ("band", "shortest", "rowcap", "contig", "leading", "n", "unmapped", "clip")
# (rowcap_rls: 145 = 9 * 16 + 1 -- a read of RL bases with two vectors per segment goes idle only at row RL + 16 + w, past the cap RL + 16)
GPU_SPEC = dict(rls=[64, 150, 240, 400], rowcap_rls=[145], n_random=300, n_reads=200, rec_rls=[64, 150, 240])

_items = {}


def class_items(ix, RL):
    """{class: [Item]} at a kernel RL, made once per process (items are compared by identity across the checks)."""
    if RL not in _items:
        _items[RL] = su.Maker(ix).classes(RL)
    return _items[RL]


def batches_at(ix, RL, n_random, only=None):
    """{batch name: [Item]}: each class with an unmapped read of RL bases in its middle, then the batch shapes over the pool of all classes."""
    mk, geo = su.Maker(ix), su.Geometry(ix)
    cls = class_items(ix, RL)
    out = {}
    for name, items in cls.items():
        if only is None or name in only:
            out["class_" + name] = items[:len(items) // 2] + [mk.pin(RL)] + items[len(items) // 2:]
    if only is not None:
        return out
    pool = [it for items in cls.values() for it in items]
    rng = np.random.default_rng(99 + RL)
    order = rng.permutation(len(pool))
    take = lambda n, start=0: [pool[order[(start + j) % len(pool)]] for j in range(n)]
    elig = su.predicate(geo, pool + [mk.pin(RL)])[:-1]
    yes = [it for it, e in zip(pool, elig) if e and it.cls != "leading"]
    no = [it for it, e in zip(pool, elig) if not e]
    assert len(yes) > 16 and len(no) >= 8
    start = 0
    for n in BATCH_SIZES:                                             # (a batch's last read pins RL: sizes as asked for, the pin included)
        out["size_%d" % n] = take(n - 1, start) + [mk.pin(RL, n)]
        start += n - 1
    shortest_k0 = [it for it in cls["shortest"] if it.k == 0 and it.want][0]
    full_k7 = [it for it in cls["rowcap"] if it.U == RL and it.k == 7][0]
    out["short_beside_full"] = [shortest_k0, full_k7] * 4
    one = [it for it in yes if it.k <= 3]; two = [it for it in yes if it.k >= 4]
    out["one_and_two_vectors"] = [x for j in range(8) for x in (one[j % len(one)], two[j % len(two)])][:15] + [mk.pin(RL, 1)]
    out["only_group_7"] = no[:6] + [mk.pin(RL, 2), full_k7]
    out["none_eligible"] = no[:7] + [mk.pin(RL, 3)]
    out["random_order"] = take(n_random - 1, 5) + [mk.pin(RL, 4)]
    return out


def all_batches(ix, spec):
    """[(RL, name, items)] of a run: every class and batch shape at spec["rls"], the row-cap class alone at spec["rowcap_rls"]."""
    out = []
    for RL in spec["rls"]:
        out += [(RL, name, items) for name, items in batches_at(ix, RL, spec["n_random"]).items()]
    for RL in spec["rowcap_rls"]:
        out += [(RL, name, items) for name, items in batches_at(ix, RL, 0, only=("rowcap",)).items()]
    return out


def run_single(ix, spec):
    """samFields over all_batches, use_m False and True.  {"RL/batch/use_m/field": array, "RL/batch/valid": [count, count]}"""
    from snap_amd.aligner import BaseAligner
    out, ctx = {}, {}
    try:
        for RL, name, items in all_batches(ix, spec):
            if RL not in ctx:
                ctx[RL] = BaseAligner(ix, abi.default_params(max_read_len=RL))
            z = su.pack(items)
            valid = []
            for use_m in (False, True):
                got = ctx[RL].samFields(z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"], z["results"], use_m)
                valid.append(ctx[RL].samf_pre_valid())
                for k in KEYS:
                    out["%d/%s/%d/%s" % (RL, name, use_m, k)] = got[k]
            out["%d/%s/valid" % (RL, name)] = np.array(valid)
    finally:
        for a in ctx.values():
            a.close()
    return out


def paired_batch(ix, RL):
    cls = class_items(ix, RL)
    return su.pair_up(su.Geometry(ix), [it for items in cls.values() for it in items])


def run_paired(ix, spec):
    """samFieldsPaired over the mapped items of every class at each RL, two by two."""
    from snap_amd.aligner import ChimericPairedEndAligner
    out = {}
    for RL in spec["rls"]:
        mates, res = paired_batch(ix, RL)
        z = su.pack(mates)
        a = ChimericPairedEndAligner(ix, abi.default_params(max_read_len=RL), abi.default_paired_params())
        try:
            valid = []
            for use_m in (False, True):
                got = a.samFieldsPaired(z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"], res, use_m)
                valid.append(a.samf_pre_valid())
                for k in PAIRED_KEYS:
                    out["%d/paired/%d/%s" % (RL, use_m, k)] = got[k]
            out["%d/paired/valid" % RL] = np.array(valid)
        finally:
            a.close()
    return out


def record_reads(ix, RL, n):
    """Reads for the aligner from the cut-and-edit recipe: 50 .. RL bases (the first one RL), 0 .. 5 edits, either direction."""
    mk = su.Maker(ix)
    rng = np.random.default_rng(5 + RL)
    bs, qs = [], []
    for i in range(n):
        U = RL if i == 0 else int(rng.integers(50, RL + 1))
        ne = int(rng.integers(0, 6))
        edits = []
        for o in sorted(rng.choice(np.arange(2, U - 12), size=ne, replace=False)):
            t = rng.random()
            edits.append(("S", int(o)) if t < 0.6 else (("I", int(o), int(rng.integers(1, 3))) if t < 0.8 else ("D", int(o), int(rng.integers(1, 3)))))
        edits = [e for j, e in enumerate(edits) if j == 0 or e[1] - edits[j - 1][1] > 3]
        b = su.cut_and_edit(mk.G, rng, mk.clean(rng, U, int(rng.integers(0, len(mk.begin)))), U, edits)
        bs.append(su.revcomp(b) if i & 1 else b); qs.append(rng.integers(35, 74, size=U).astype(np.uint8))
    offs = np.concatenate([[0], np.cumsum([b.size for b in bs])]).astype(np.uint64)
    return np.concatenate(bs), np.concatenate(qs), offs


def run_records(ix, spec):
    """alignSamRecords with no secondary options (one record per read) over record_reads."""
    from snap_amd.aligner import BaseAligner
    out = {}
    for RL in spec["rec_rls"]:
        bases, quals, offs = record_reads(ix, RL, spec["n_reads"])
        n = offs.size - 1
        dl = np.diff(offs.astype(np.int64)).astype(np.int32)
        a = BaseAligner(ix, abi.default_params(max_k=8, max_read_len=RL))
        try:
            valid = []
            for use_m in (False, True):
                rec = a.alignSamRecords(bases, quals, offs, np.zeros(n, np.int32), dl, np.zeros(n, np.uint8), use_m=use_m)
                valid.append(a.samf_pre_valid())
                assert not rec["truncated"] and rec["n_records"] == n
                for k in REC_KEYS:
                    out["%d/records/%d/%s" % (RL, use_m, k)] = rec[k]
                out["%d/records/%d/results" % (RL, use_m)] = rec["results"].view(np.uint8)
            out["%d/records/valid" % RL] = np.array(valid)
        finally:
            a.close()
    return out


def run_all(ix, spec):
    """The three runs in one (their keys do not collide: no batch is called "paired" or "records")."""
    out = run_single(ix, spec)
    out.update(run_paired(ix, spec))
    out.update(run_records(ix, spec))
    return out


RUNNERS = dict(single=run_single, paired=run_paired, records=run_records, all=run_all)


def child_main(mode, spec_json, out_path, lib_path):
    """Run in a process of its own (SNAPGPU_SAMF_DP8 is read once per process): the same run, saved for the parent to compare."""
    if lib_path:
        import snap_amd.aligner as al
        al.LIB_PATH, al._lib = lib_path, None
    np.savez(out_path, **RUNNERS[mode](util.load_golden_index(), json.loads(spec_json)))
    print("samf child", mode, "done")


def run_child(mode, spec, out_path, lib_path, dp8="0", timeout=3000):
    code = "from tests.test_zz_gpu_samf_prepass import child_main as f; f(%r, %r, %r, %r)" % (mode, json.dumps(spec), str(out_path), lib_path)
    r = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", code], cwd=util.ROOT, env=dict(os.environ, SNAPGPU_SAMF_DP8=dp8),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, stdin=subprocess.DEVNULL, timeout=timeout)
    assert r.returncode == 0 and b"samf child" in r.stdout, r.stdout.decode(errors="replace")[-4000:]
    return dict(np.load(str(out_path)))


def check_on_equals_off(on, off):
    """Every array of the run with the pre-pass == the run without it (off: that run, or run_all's, which holds it); without it no SamfPre
    record is valid."""
    assert len(on) > 0 and not set(on) - set(off), sorted(set(on) - set(off))[:8]
    for key in sorted(on):
        if key.endswith("/valid"):
            assert (off[key] == 0).all(), (key, off[key])
            continue
        a, b = on[key], off[key]
        assert a.shape == b.shape, key
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, (key, bad[:8], a[bad[:3]], b[bad[:3]])


def check_who_took_the_prepass(ix, spec, on):
    """After each samFields call the valid count is the predicate's, exactly; every class meant to be eligible has eligible items, every item
    says what its class means it to.  Returns {(RL, class): (eligible, items)}."""
    geo = su.Geometry(ix)
    table = {}
    for RL, name, items in all_batches(ix, spec):
        assert su.kernel_rl([it.U for it in items]) == RL, (RL, name)
        el = su.predicate(geo, items)
        want = su.expected_valid(geo, items)
        got = on["%d/%s/valid" % (RL, name)]
        print("valid SamfPre records: RL %3d %-22s items %3d predicate %3d launched %d kernel %s" % (RL, name, len(items), int(el.sum()), su.prepass_launched(RL), got.tolist()))
        assert (got == want).all(), (RL, name, got, want)
        if name.startswith("class_"):
            table[(RL, name[6:])] = (int(el.sum()), len(items))
            if name[6:] in ELIGIBLE_CLASSES:
                assert el.any(), (RL, name)
            for it, e in zip(items, el):
                assert it.want is None or it.want == bool(e), (RL, name, it.tag, it.want, e)
        elif name == "only_group_7":
            assert el.tolist() == [False] * 7 + [True]
        elif name == "none_eligible":
            assert not el.any()
        elif name == "short_beside_full":
            assert el.all()
        elif name == "one_and_two_vectors":
            assert el[:-1].all() and [it.k >= 4 for it in items[:-1]] == [bool(j & 1) for j in range(len(items) - 1)]
    # the launch is what the predicate assumes: on up to 240 bases, off beyond
    assert su.prepass_launched(64) and su.prepass_launched(240) and not su.prepass_launched(241) and not su.prepass_launched(400)
    return table


def check_no_prepass_without_affine_gap(ix, RL=64):
    from snap_amd.aligner import BaseAligner
    items = batches_at(ix, RL, 0, only=("band",))["class_band"]
    z = su.pack(items)
    a = BaseAligner(ix, abi.default_params(max_read_len=RL, use_affine_gap=0))
    try:
        a.samFields(z["bases"], z["quals"], z["offsets"], z["front_clip"], z["data_len"], z["results"])
        assert a.samf_pre_valid() == 0
    finally:
        a.close()
    assert su.expected_valid(su.Geometry(ix), items, use_affine_gap=False) == 0 and su.expected_valid(su.Geometry(ix), items) > 0


def strip_clips(ops, n_ops):
    """(soft clip in front, the ops between, soft clip behind) of a record's CIGAR"""
    o = [int(x) for x in ops[:max(int(n_ops), 0)]]
    front = back = 0
    if o and o[0] & 15 == 4:
        front, o = o[0] >> 4, o[1:]
    if o and o[-1] & 15 == 4:
        back, o = o[-1] >> 4, o[:-1]
    return front, o, back


def check_properties(lengths, got):
    """cigar_properties on every mapped record (soft clips taken off: it speaks of the aligned part), and the whole CIGAR spans the whole read
    (lengths: each record's unclipped read length)."""
    n = len(lengths)
    inner = dict(n_ops=np.zeros(n, np.int32), ops=np.zeros_like(got["ops"]), edit_distance=got["nm"], extra_clipped_after=np.zeros(n, np.int64))
    length = np.zeros(n, np.int64)
    for i, U in enumerate(lengths):
        if got["flag"][i] & 4 or got["n_ops"][i] <= 0:
            assert got["n_ops"][i] == -1
            continue
        front, o, back = strip_clips(got["ops"][i], got["n_ops"][i])
        inner["n_ops"][i] = len(o); inner["ops"][i, :len(o)] = o
        length[i] = int(U) - front - back
        assert length[i] > 0, i
    cigar_properties(inner, length, np.zeros(n, np.int64))


def check_single_properties(ix, spec, on):
    mapped = 0
    for RL, name, items in all_batches(ix, spec):
        for use_m in (0, 1):
            got = {k: on["%d/%s/%d/%s" % (RL, name, use_m, k)] for k in KEYS}
            check_properties([it.U for it in items], got)
            mapped += int((got["flag"] & 4 == 0).sum())
            if name == "class_leading":                       # the record a retry finished: mapped with a CIGAR over the whole read (above), or unmapped
                assert ((got["flag"] & 4 != 0) == (got["n_ops"] == -1)).all()
    assert mapped > 100


def reference_index(ix, tmp_path):
    """The compiled reference over the golden genome (as tests/test_zz_gpu_cigar.py: test_compute_cigar_ag_vs_live_reference), or None."""
    from oracle import ref
    if not ref.available() or not os.path.exists(ref.CLI_PATH):
        return None
    from snap_amd import synth
    from snap_amd.index import GenomeIndex
    from tests.test_zz_gpu_paired_sam_onecall import golden_contigs
    G = ix.genome
    cb = [int(x) for x in ix.contig_begin] + [int(ix.n_bases)]
    contigs = [(c.name, G[cb[i]:cb[i + 1] - ix.chromosome_padding].copy()) for i, c in enumerate(ix.contigs)]
    assert all((s != ord("n")).all() for _, s in contigs) and len(golden_contigs(ix)) == len(contigs)
    fa = str(tmp_path / "ref.fa"); synth.write_fasta(fa, contigs)
    alt = [c.name for c in ix.contigs if c.is_alt]
    ref.build_index(fa, str(tmp_path / "idx"), ix.seed_len, threads=4, extra=sum((["-altContigName", a] for a in alt), []))
    ix2 = GenomeIndex.load_from_directory(str(tmp_path / "idx"))
    assert (ix2.contig_begin == ix.contig_begin).all() and (ix2.genome_padded == ix.genome_padded).all()
    return ref.RefIndex(str(tmp_path / "idx"))


def check_against_reference(ix, spec, on, ri):
    """Every predicate-eligible item outside the leading-indel class: the record's CIGAR without its soft clips and its NM are the
    reference's ops and edit distance for the oriented, clipped pattern at loc with limit k; the soft clips are the constructed ones plus
    the reference's tail insertion (and what it clipped at the contig's end); POS is loc in its contig."""
    geo = su.Geometry(ix)
    n_checked = 0
    for RL, name, items in all_batches(ix, spec):
        if not name.startswith("class_") or name == "class_leading":
            continue
        el = su.predicate(geo, items)
        sel = [i for i in range(len(items)) if el[i]]
        if not sel:
            continue
        pats = [items[i].pattern for i in sel]
        data = np.concatenate(pats); q = np.concatenate([items[i].pattern_quals for i in sel])
        length = np.array([p.size for p in pats], np.int32)
        off = np.zeros(len(sel), np.uint64); off[1:] = np.cumsum(length)[:-1]
        loc = np.array([items[i].loc for i in sel], np.int64); k = np.array([items[i].k for i in sel], np.int32)
        for use_m in (0, 1):
            exp = ri.compute_cigar_ag(data, q, off, length, loc, np.zeros(len(sel), np.int32), k, bool(use_m), fresh_object=True, ops_stride=64)
            got = {f: on["%d/%s/%d/%s" % (RL, name, use_m, f)] for f in KEYS}
            for j, i in enumerate(sel):
                it, who = items[i], (RL, name, items[i].tag, use_m)
                assert exp["add_front_clipping"][j] == 0 and exp["edit_distance"][j] >= 0, (who, "the helper made a leading indel or a pattern the reference refuses")
                assert got["flag"][i] & 4 == 0 and (got["flag"][i] & 16 != 0) == (int(it.res["direction"]) == 1), who
                front, o, back = strip_clips(got["ops"][i], got["n_ops"][i])
                assert o == [int(x) for x in exp["ops"][j, :exp["n_ops"][j]]], (who, util.cigar_text(got["ops"][i], got["n_ops"][i]), util.cigar_text(exp["ops"][j], exp["n_ops"][j]))
                assert got["nm"][i] == exp["edit_distance"][j], who
                assert front == it.bcb and back == it.bca + int(exp["back_clipping_missed"][j]) + int(exp["extra_clipped_after"][j]), (who, front, back)
                c = geo.contig_at(it.loc)
                assert got["contig"][i] == c and got["pos"][i] == it.loc - geo.begin[c] + 1 and got["mapq"][i] == int(it.res["mapq"]), who
                n_checked += 1
    return n_checked


def check_paired_against_single(ix, spec, single, paired):
    """k_samf_dp8_paired: the valid count is the predicate's over the mates; each mate's CIGAR and NM are what samFields gave for the same item
    alone, wherever the read does not hang over its contig's end (extra == 0)."""
    geo = su.Geometry(ix)
    n_same = 0
    for RL in spec["rls"]:
        mates, _ = paired_batch(ix, RL)
        assert len(mates) > 50 and su.kernel_rl([it.U for it in mates]) == RL
        want = su.expected_valid(geo, mates)
        assert (paired["%d/paired/valid" % RL] == want).all(), (RL, paired["%d/paired/valid" % RL], want)
        print("valid SamfPre records: RL %3d paired mates %3d predicate %3d kernel %s" % (RL, len(mates), int(su.predicate(geo, mates).sum()), paired["%d/paired/valid" % RL].tolist()))
        where = {}
        for name, items in batches_at(ix, RL, 0, only=tuple(class_items(ix, RL))).items():
            for i, it in enumerate(items):
                where[id(it)] = (name, i)
        for use_m in (0, 1):
            got = {k: paired["%d/paired/%d/%s" % (RL, use_m, k)] for k in PAIRED_KEYS}
            check_properties([it.U for it in mates], got)
            for m, it in enumerate(mates):
                c = geo.contig_at(it.loc)
                if c < 0 or it.loc + it.data_len > geo.contig_end(c):
                    continue
                name, i = where[id(it)]
                for k in ("n_ops", "nm", "ops"):
                    assert (got[k][m] == single["%d/%s/%d/%s" % (RL, name, use_m, k)][i]).all(), (RL, it.cls, it.tag, use_m, k)
                n_same += 1
    assert n_same > 100


def check_records_valid(ix, spec, rec):
    """k_samf_dp8_rec: the valid count is the predicate's over the returned results of the (primary) records; cigar_properties on each."""
    geo = su.Geometry(ix)
    for RL in spec["rec_rls"]:
        _, _, offs = record_reads(ix, RL, spec["n_reads"])
        U = np.diff(offs.astype(np.int64))
        assert su.kernel_rl(U) == RL
        for use_m in (0, 1):
            res = rec["%d/records/%d/results" % (RL, use_m)].view(abi.RESULT_DTYPE)
            kind, rd = rec["%d/records/%d/rec_kind" % (RL, use_m)], rec["%d/records/%d/rec_read" % (RL, use_m)]
            assert (kind == 0).all() and (rd == np.arange(U.size)).all()
            el = np.array([su.eligible(geo, RL, int(U[i]), 0, int(U[i]), res[i]) for i in rd])
            want = int(el.sum()) if su.prepass_launched(RL) else 0
            got = int(rec["%d/records/valid" % RL][use_m])
            print("valid SamfPre records: RL %3d records %3d aligned %3d predicate %3d kernel %d" % (RL, U.size, int((res["status"] != 0).sum()), int(el.sum()), got))
            assert got == want and int(el.sum()) > U.size // 4, (RL, got, want)
            got = {k: rec["%d/records/%d/%s" % (RL, use_m, k)] for k in KEYS}
            assert ((got["flag"] & 4 == 0) == (res["status"] != 0)).sum() >= U.size - 2
            check_properties(U[rd], got)


# ------------------------------------------------------------------------------------------------------------------------ the GPU tests
@pytest.fixture(scope="module")
def single_on(golden_index):
    return run_single(golden_index, GPU_SPEC)


@pytest.fixture(scope="module")
def all_off(tmp_path_factory):
    """run_all in ONE child process without the pre-pass, shared by the three on == off tests."""
    import snap_amd.aligner as al
    return run_child("all", GPU_SPEC, tmp_path_factory.mktemp("samf") / "off.npz", al.LIB_PATH)


@pytest.mark.gpu
def test_valid_count_is_the_predicates(golden_index, single_on):
    table = check_who_took_the_prepass(golden_index, GPU_SPEC, single_on)
    assert all(table[(RL, c)][0] > 0 for RL in GPU_SPEC["rls"] for c in ELIGIBLE_CLASSES)
    check_no_prepass_without_affine_gap(golden_index)


@pytest.mark.gpu
def test_single_end_with_the_prepass_equals_without(golden_index, single_on, all_off):
    check_on_equals_off(single_on, all_off)


@pytest.mark.gpu
def test_records_satisfy_the_cigar_properties(golden_index, single_on):
    check_single_properties(golden_index, GPU_SPEC, single_on)


@pytest.mark.gpu
def test_eligible_records_equal_the_reference(golden_index, single_on, tmp_path):
    ri = reference_index(golden_index, tmp_path)
    if ri is None:
        pytest.skip("oracle/_ref not on this box")
    assert check_against_reference(golden_index, GPU_SPEC, single_on, ri) > 400


@pytest.mark.gpu
def test_paired_mates_with_the_prepass(golden_index, single_on, all_off):
    on = run_paired(golden_index, GPU_SPEC)
    check_paired_against_single(golden_index, GPU_SPEC, single_on, on)
    check_on_equals_off(on, all_off)


@pytest.mark.gpu
def test_record_list_with_the_prepass(golden_index, all_off):
    on = run_records(golden_index, GPU_SPEC)
    check_records_valid(golden_index, GPU_SPEC, on)
    check_on_equals_off(on, all_off)
