"""Shared by the record-list tests (snapgpu_align_sam_single_records): the option sets of tests/golden/sam_records_single.npz
(scripts/make_golden_sam_records.py), one call of the library per set, and the field-for-field comparison with what the reference CLI
printed."""
import os

import numpy as np

from snap_amd import abi
from tests import util

# tag -> (reference command line, snapgpu_params fields, (om, omax, mpc) or None, -ae, use_m)
SETS = {
    "om1_omax4": (["-om", "1", "-omax", "4"], {}, (1, 4, -1), 0, 1),
    "D2_om2_mpc2": (["-D", "2", "-om", "2", "-mpc", "2"], dict(extra_search_depth=2), (2, 0x7fffffff, 2), 0, 1),
    "ea_om1": (["-ea", "-om", "1"], dict(emit_alt_alignments=1), (1, 0x7fffffff, -1), 0, 1),
    "ea": (["-ea"], dict(emit_alt_alignments=1), None, 0, 1),
    "ae": (["-ae"], {}, None, 1, 1),
    "ae_om1": (["-ae", "-om", "1"], {}, (1, 0x7fffffff, -1), 1, 1),
    "lvonly_eqx_om1": (["-G-", "-=", "-om", "1"], dict(use_affine_gap=0), (1, 0x7fffffff, -1), 0, 0),
}
FIELDS = ("flag", "contig", "pos", "mapq", "nm", "n_ops")


def fixture():
    return np.load(os.path.join(util.GOLDEN, "sam_records_single.npz"))


def skip_mask(bases, offsets, front_clip, data_len, max_k, min_read_len=50):
    """The reads the reference does not give to its aligner (SingleAligner.cpp:211-232): shorter than -mrl after clipping, or more Ns than -d."""
    n = offsets.size - 1
    skip = np.zeros(n, np.uint8)
    for i in range(n):
        b = bases[int(offsets[i]) + int(front_clip[i]):int(offsets[i]) + int(front_clip[i]) + int(data_len[i])]
        skip[i] = 1 if (data_len[i] < min_read_len or int((b == ord("N")).sum()) > max_k) else 0
    return skip


def make_aligner(index, tag, max_read_len=400, device=0, params_kw=None):
    from snap_amd.aligner import BaseAligner
    cli, kw, sec, ae, use_m = SETS[tag]
    kw = dict(kw); kw.update(params_kw or {})
    a = BaseAligner(index, abi.default_params(max_read_len=max_read_len, **kw), device=device)
    if sec is not None:
        a.enable_secondary(sec[0], max_results=sec[1], max_per_contig=sec[2], adjust_alignments=ae)
    return a


def run_set(index, tag, bases, quals, offsets, front_clip, data_len, **call_kw):
    """One snapgpu_align_sam_single_records call for option set `tag`; returns BaseAligner.alignSamRecords' dict."""
    cli, kw, sec, ae, use_m = SETS[tag]
    a = make_aligner(index, tag)
    try:
        skip = skip_mask(bases, offsets, front_clip, data_len, int(a.params.max_k))
        return a.alignSamRecords(bases, quals, offsets, front_clip, data_len, skip, use_m=bool(use_m), adjust_primary=bool(ae and sec is None), **call_kw)
    finally:
        a.close()


def compare(exp, got, n_reads, verbose=True):
    """exp: dict(rec_read, flag, contig, pos, mapq, nm, n_ops, ops) in the reference's file order; got: alignSamRecords' dict.
    Returns (problems, reads left out).  The record list itself -- how many records, which read each belongs to, in which order -- is
    compared for every read; the fields of a read's records are left out only when the library flags one of them
    reference_history_dependent (the reference's own answer depends on what its aligner object did before)."""
    problems = []
    if got["n_records"] != exp["rec_read"].size or got["rec_read"].size != exp["rec_read"].size:
        return ["%d records, the reference wrote %d" % (got["n_records"], exp["rec_read"].size)], 0
    if not (got["rec_read"] == exp["rec_read"]).all():
        k = int(np.flatnonzero(got["rec_read"] != exp["rec_read"])[0])
        return ["record %d belongs to read %d, the reference's to read %d" % (k, got["rec_read"][k], exp["rec_read"][k])], 0
    begin = np.concatenate([[0], np.cumsum(np.bincount(exp["rec_read"], minlength=n_reads))])
    if not (got["rec_begin"].astype(np.int64) == begin).all():
        problems.append("rec_begin is not the running count of the records")
    left_out = np.unique(got["rec_read"][got["stale"] != 0])
    keep = ~np.isin(got["rec_read"], left_out)
    for r in np.flatnonzero(keep):
        bad = [f for f in FIELDS if int(got[f][r]) != int(exp[f][r])]
        m = int(exp["n_ops"][r])
        if m > 0 and not bad and not (got["ops"][r, :m] == exp["ops"][r, :m]).all():
            bad.append("ops")
        if bad:
            problems.append("record %d (read %d, kind %d): %s" % (r, got["rec_read"][r], got["rec_kind"][r],
                                                                   ", ".join("%s %s != %s" % (f, got[f][r] if f != "ops" else util.cigar_text(got["ops"][r], got["n_ops"][r]),
                                                                                                exp[f][r] if f != "ops" else util.cigar_text(exp["ops"][r], exp["n_ops"][r])) for f in bad)))
    # kinds: the first record of a read is its primary, then its n_secondary secondary results, then -- last -- its first-ALT record, which
    # exists exactly where the call's first_alt result is not NotFound
    first = np.zeros(got["rec_read"].size, bool); first[begin[:-1][begin[:-1] < first.size]] = True
    if not ((got["rec_kind"] == 0) == first).all():
        problems.append("rec_kind 0 is not exactly the first record of each read")
    kind = got["rec_kind"]; rd = got["rec_read"]
    if not (np.bincount(rd[kind == 1], minlength=n_reads) == got["n_secondary"]).all():
        problems.append("the records of kind 1 of a read are not as many as its n_secondary")
    n_alt = np.bincount(rd[kind == 2], minlength=n_reads)
    if not (n_alt == (got["first_alt"]["status"] != 0)).all():
        problems.append("a record of kind 2 exists where first_alt is NotFound, or is missing where it is not")
    last = np.zeros(kind.size, bool); last[begin[1:][begin[1:] > begin[:-1]] - 1] = True
    if not last[kind == 2].all() or (kind > 2).any():
        problems.append("a record of kind 2 is not its read's last")
    pos_in_read = np.arange(kind.size) - begin[rd]
    if not (pos_in_read[kind == 1] <= got["n_secondary"][rd[kind == 1]]).all():
        problems.append("a record of kind 1 comes after its read's first-ALT record")
    if not (((got["flag"] & 0x100) != 0) == ~first)[keep].all():
        problems.append("0x100 is not exactly on the records that are not their read's first")
    if verbose and problems:
        print("\n".join(problems[:20]))
    return problems, int(left_out.size)


def expected(z, tag):
    return {k: z["%s_%s" % (tag, k)] for k in ("rec_read",) + FIELDS + ("ops",)}


def clipped_read_at_contig_end(index, length=100, tail=10):
    """One read the reader clips ('#' tail) that aligns up to the last base of the first contig: what -ae refuses (adjust.h's limitation,
    include/snapgpu.h: snapgpu_adjust_alignments), together with an ordinary read before and after it."""
    from snap_amd.index import GENOME_PAD
    z = fixture()
    G = index.genome_padded[GENOME_PAD:GENOME_PAD + index.n_bases]
    real_end = int(index.contig_begin[1]) - int(index.chromosome_padding)
    o = z["offsets"].astype(np.int64)
    rb = [z["bases"][o[0]:o[1]], np.char.upper(np.ascontiguousarray(G[real_end - length:real_end]).view("S1")).view(np.uint8), z["bases"][o[20]:o[21]]]
    rq = [z["quals"][o[0]:o[1]], np.concatenate([np.full(length - tail, ord("I"), np.uint8), np.full(tail, ord("#"), np.uint8)]), z["quals"][o[20]:o[21]]]
    offsets = np.concatenate([[0], np.cumsum([b.size for b in rb])]).astype(np.uint64)
    fc = np.zeros(3, np.int32); dl = np.array([rb[0].size, length - tail, rb[2].size], np.int32)
    return np.concatenate(rb), np.concatenate(rq), offsets, fc, dl


def check_ae_refusal(index):
    """-ae, with and without secondary results: the batch with the clipped contig-end read is refused as a whole (SNAPGPU_E_UNSUPPORTED, a
    message that starts with "-ae:", which snapgpu-sam matches), the same batch with that read unclipped is answered, and so is the clipped
    one without -ae."""
    from snap_amd.aligner import SnapGpuError
    import pytest
    bases, quals, offsets, fc, dl = clipped_read_at_contig_end(index)
    for tag in ("ae", "ae_om1"):
        with pytest.raises(SnapGpuError, match=r"failed \(-3\): -ae:"):
            run_set(index, tag, bases, quals, offsets, fc, dl)
        q2 = quals.copy(); q2[q2 == ord("#")] = ord("I")
        dl2 = np.diff(offsets.astype(np.int64)).astype(np.int32)
        ok = run_set(index, tag, bases, q2, offsets, fc, dl2)
        assert ok["n_records"] >= 3 and (ok["flag"][ok["rec_read"] == 1][0] & 4) == 0
    ok = run_set(index, "om1_omax4", bases, quals, offsets, fc, dl)
    assert ok["n_records"] >= 3 and (ok["flag"][ok["rec_read"] == 1][0] & 4) == 0


def check_device_form(index, hb, n=300):
    """snapgpu_align_sam_single_records_device == the host form, bit for bit: with every optional result array (a context with secondary
    results and first-ALT records, an overflow rerun inside), with none of them (the library's own scratch), on a context without secondary
    results (n_secondary zeroed), with a capacity that is too small, and with no reads."""
    z = fixture()
    o = z["offsets"][:n + 1]
    bases, quals, fc, dl = z["bases"][:int(o[-1])], z["quals"][:int(o[-1])], z["front_clip"][:n], z["data_len"][:n]
    per_record = ("rec_read", "rec_kind", "flag", "contig", "pos", "mapq", "n_ops", "nm", "ops", "stale")
    for tag, with_results in (("ea_om1", True), ("ea_om1", False), ("ae", True), ("om1_omax4", False)):
        cli, kw, sec, ae, use_m = SETS[tag]
        host = run_set(index, tag, bases, quals, o, fc, dl, secondary_stride=4)
        a = make_aligner(index, tag)
        try:
            skip = skip_mask(bases, o, fc, dl, int(a.params.max_k))
            for cap in (host["n_records"] + 7, host["n_records"] // 2):
                like = dict(rec_begin=np.zeros(n + 1, np.uint64), rec_read=np.zeros(cap, np.uint32), rec_kind=np.zeros(cap, np.uint8), flag=np.zeros(cap, np.int32),
                            contig=np.zeros(cap, np.int32), pos=np.zeros(cap, np.int64), mapq=np.zeros(cap, np.int32), ops=np.zeros((cap, 64), np.uint32),
                            n_ops=np.zeros(cap, np.int32), nm=np.zeros(cap, np.int32), stale=np.zeros(cap, np.int32))
                res_like = dict(results=np.zeros(n, abi.RESULT_DTYPE), first_alt=np.zeros(n, abi.RESULT_DTYPE), secondary=np.zeros((n, 4), abi.RESULT_DTYPE),
                                n_secondary=np.full(n, 0xCDCDCDCD, np.uint32))
                d = {k: hb.upload(v) for k, v in like.items()}
                dr = {k: hb.upload(v) for k, v in res_like.items()} if with_results else {k: 0 for k in res_like}
                d_in = [hb.upload(np.concatenate([x, np.zeros(16, np.uint8)])) for x in (bases, quals)] + [hb.upload(x) for x in (o, fc, dl, skip)]
                n_rec, truncated = a.alignSamRecords_device(n, 160, *d_in, cap, d["rec_begin"], d["rec_read"], d["rec_kind"], d["flag"], d["contig"], d["pos"], d["mapq"],
                                                            d["ops"], 64, d["n_ops"], d["nm"], d["stale"], use_m=bool(use_m), adjust_primary=bool(ae and sec is None),
                                                            d_results=dr["results"], d_first_alt=dr["first_alt"], d_secondary=dr["secondary"],
                                                            secondary_stride=4 if with_results else 0, d_n_secondary=dr["n_secondary"])
                assert n_rec == host["n_records"] and truncated == (cap < n_rec), (tag, cap, n_rec)
                m = min(cap, n_rec)
                assert (hb.download(d["rec_begin"], like["rec_begin"]) == host["rec_begin"]).all()
                for k in per_record:
                    assert (hb.download(d[k], like[k])[:m] == host[k][:m]).all(), (tag, with_results, cap, k)
                if with_results:
                    for k in ("results", "first_alt", "n_secondary"):
                        assert hb.download(dr[k], res_like[k]).tobytes() == host[k].tobytes(), (tag, k)
                    if sec is not None:
                        assert hb.download(dr["secondary"], res_like["secondary"]).tobytes() == host["secondary"].tobytes(), tag
            d0 = hb.upload(np.full(1, 7, np.uint64))                 # no reads: rec_begin[0] = 0, nothing else touched
            assert a.alignSamRecords_device(0, 160, 0, 0, 0, 0, 0, 0, 0, d0, *([0] * 7), 64, 0, 0, 0) == (0, False)
            assert int(hb.download(d0, np.zeros(1, np.uint64))[0]) == 0
        finally:
            a.close()
            hb.free_all()
