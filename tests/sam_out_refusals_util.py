"""What the 17 SAM / BAM / BGZF output calls of the C ABI answer to a call they refuse, and to the smallest calls they accept: the return code,
the text of snapgpu_last_error and every output word afterwards, one table row each.  Shared by tests/test_emu_sam_out_refusals.py (the
wavefront emulator) and tests/test_zz_gpu_sam_out_refusals.py (the GPU).  The table was written by running `python -m
tests.sam_out_refusals_util tests/emu/_build/libsnapgpu_emu.so` on the emulated library of the commit before the host layer of these calls was
folded into one body: it states what that library answered, and a row changes only when the ABI is meant to.

A row is (call, defect, return code, message, outputs).  The call starts from arguments that are accepted (3 reads / 6 records of
bam_util.handcrafted, 2 pairs / 2 units of bam_util.handcrafted_pairs, 3 golden reads, 2 golden pairs) on a context that has its contig names
and BAM numbers; the defect (DEFECTS below, several joined by "+") changes them.  Every output word starts as SENT; `outputs` lists the words
that hold something else afterwards (of an array: its first word).  A row with a message launches nothing."""
import ctypes as C
import os

import numpy as np

from tests import util

SENT = 0x7777777777777777
OPTIONAL = ("rec_read", "unit_pair", "results", "first_alt", "stream")
HOST_WORDS = ("text_bytes", "n_records", "n_members", "bgzf_bytes", "bam_bytes", "out_bytes")      # host words in the device forms too
OUT_ARRAYS = ("line_begin", "rec_begin", "member_begin")
COUNTS = ("n_records", "n_units", "n", "n_pairs", "n_bytes")

_RECS = "bases quals offsets names name_off %s flag contig pos mapq ops ops_stride:u32 n_ops nm"
_MATES = " rnext pnext tlen first_written"
_TEXT = " text_capacity:u64 text line_begin text_bytes"
_BGZF = " block_input:u32 bgzf_capacity:u64 bgzf member_begin member_capacity:u64 n_members bgzf_bytes bam_bytes"
_SINGLE = "ctx n:u32 bases quals offsets front_clip data_len skip use_m:int adjust_primary:int names name_off ops_stride:u32 record_capacity:u64 n_records:out rec_begin flag"
_PAIRED = "ctx n_pairs:u32 bases quals offsets front_clip data_len skip use_m:int names name_off ops_stride:u32 results first_alt flag first_written"
SIGNATURES = {
    "snapgpu_sam_text_single": "ctx n_records:u64 n_reads:u32 " + _RECS % "rec_read" + _TEXT,
    "snapgpu_sam_text_single_device": "ctx n_records:u64 " + _RECS % "rec_read" + _TEXT + " stream",
    "snapgpu_sam_text_paired": "ctx n_units:u64 n_pairs:u32 " + _RECS % "unit_pair" + _MATES + _TEXT,
    "snapgpu_sam_text_paired_device": "ctx n_units:u64 " + _RECS % "unit_pair" + _MATES + _TEXT + " stream",
    "snapgpu_align_sam_single_text": _SINGLE + _TEXT,
    "snapgpu_align_sam_paired_text": _PAIRED + _TEXT,
    "snapgpu_align_sam_single_bgzf": _SINGLE + _BGZF,
    "snapgpu_align_sam_paired_bgzf": _PAIRED + _BGZF,
    "snapgpu_align_sam_paired": "ctx n_pairs:u32 bases quals offsets front_clip data_len skip use_m:int results first_alt flag contig pos mapq ops ops_stride:u32 n_ops nm"
                                + _MATES + " reference_history_dependent",
    "snapgpu_bgzf_compress": "ctx n_bytes:u64 in block_input:u32 out_capacity:u64 out member_begin n_members out_bytes",
    "snapgpu_bgzf_compress_device": "ctx n_bytes:u64 in block_input:u32 out_capacity:u64 out member_begin n_members out_bytes stream",
}
for _k in ("single", "single_device", "paired", "paired_device"):            # the BAM calls take what the text calls take (bytes / block_begin / bam_bytes
    SIGNATURES["snapgpu_bam_records_" + _k] = SIGNATURES["snapgpu_sam_text_" + _k]      # are text / line_begin / text_bytes here)
for _k in ("single", "paired"):
    SIGNATURES["snapgpu_align_sam_%s_bam" % _k] = SIGNATURES["snapgpu_align_sam_%s_text" % _k]
CALLS = sorted(SIGNATURES)
assert len(CALLS) == 17
_CTYPES = {"u32": C.c_uint32, "u64": C.c_uint64, "int": C.c_int}


def signature(call):
    """[(argument name, ctypes type of a scalar or None for a pointer)]; n_records of the fused single-end calls is a pointer (":out")"""
    return [(a.split(":")[0], _CTYPES.get(a.split(":")[1]) if ":" in a else None) for a in SIGNATURES[call].split()]


def is_paired(call):
    return "_paired" in call


def is_bam(call):
    return "_bam" in call or call.endswith("_bgzf")


def is_fused(call):
    return call.startswith("snapgpu_align_sam_")


# ---------------------------------------------------------------------------------------------------------------- the contexts
class Contexts:
    """the contexts the rows name: "single" / "paired" with contig names and BAM numbers, "bare_single" / "bare_paired" without either,
    "paired_secondary" (snapgpu_enable_paired and snapgpu_enable_secondary); made when first asked for"""

    def __init__(self):
        self.made = {}
        self.index = {"single": util.load_golden_index(), "paired": util.load_golden_index("paired_index.npz")}

    def get(self, key):
        from snap_amd import abi
        from snap_amd.aligner import BaseAligner, ChimericPairedEndAligner
        from tests import bam_util as bu
        from tests.samtext_util import contig_names_of
        if key not in self.made:
            kind = "paired" if "paired" in key else "single"
            index = self.index[kind]
            p = abi.default_params(max_k=8, max_read_len=160)
            a = ChimericPairedEndAligner(index, p, abi.default_paired_params()) if kind == "paired" else BaseAligner(index, p)
            if not key.startswith("bare"):
                a.setContigNames(contig_names_of(index)); a.setContigBamIds(bu.ref_ids(len(index.contigs)))
            if key == "paired_secondary":
                a.enable_secondary(1, max_results=3)
            self.made[key] = a
        return self.made[key]

    def close(self):
        for a in self.made.values():
            a.close()
        self.made = {}


# ---------------------------------------------------------------------------------------------------------------- accepted arguments
def _words(n):
    return np.full(n, SENT, np.uint64)


def accepted(call, ctxs):
    """{argument: numpy array, int or None} of a call that is accepted, and the context it goes to"""
    from tests import bam_util as bu
    from tests.samtext_util import pack
    paired = is_paired(call)
    key = "paired" if paired else "single"
    a = {"ctx": True, "stream": None}
    if call.startswith("snapgpu_bgzf_compress"):
        a.update({"n_bytes": 600, "in": np.frombuffer(b"ACGTTGCAAGGCTA" * 43, np.uint8)[:600].copy(), "block_input": 256, "out_capacity": 1024,
                  "out": np.zeros(1024, np.uint8), "member_begin": _words(4), "n_members": _words(1), "out_bytes": _words(1)})
        return a, key
    if not is_fused(call):
        n_contigs = len(ctxs.index[key].contigs)
        h = bu.handcrafted_pairs(n_contigs) if paired else bu.handcrafted(n_contigs)
        n_reads, n_rec = (4, 4) if paired else (3, 6)
        o = h["offsets"][:n_reads + 1]; no = h["name_off"][:n_reads + 1]
        a.update(bases=h["bases"][:int(o[-1])].copy(), quals=h["quals"][:int(o[-1])].copy(), offsets=o.copy(), names=h["names"][:int(no[-1])].copy(), name_off=no.copy())
        a.update({k: h[k][:n_rec].copy() for k in (bu.PAIR_FIELDS if paired else bu.FIELDS)})
        a.update(ops_stride=bu.OPS_STRIDE, text_capacity=4096, text=np.zeros(4096, np.uint8), line_begin=_words(n_rec + 1), text_bytes=_words(1))
        if paired:
            a.update(n_units=2, n_pairs=2, unit_pair=h["unit_pair"][:2].copy(), first_written=h["first_written"][:2].copy())
        else:
            a.update(n_records=6, n_reads=3, rec_read=h["rec_read"][:6].copy())
        return a, key
    if paired:
        z = np.load(os.path.join(util.GOLDEN, "paired_reads.npz"))
        n = 4
        o = z["o150"][:n + 1].astype(np.uint64)
        a.update(n_pairs=2, bases=z["b150"][:int(o[-1])].copy(), quals=z["q150"][:int(o[-1])].copy(), skip=np.zeros(2, np.uint8))
    else:
        z = np.load(os.path.join(util.GOLDEN, "tiny_reads.npz"))
        n = 3
        o = np.arange(n + 1, dtype=np.uint64) * 100
        a.update(n=3, bases=z["b100"][:n].reshape(-1).copy(), quals=z["q100"][:n].reshape(-1).copy(), skip=np.zeros(n, np.uint8), adjust_primary=0,
                 record_capacity=8, n_records=_words(1), rec_begin=_words(n + 1), flag=np.zeros(8, np.int32))
    nb, noff = pack([b"r%d" % i for i in range(n)])
    a.update(offsets=o, front_clip=np.zeros(n, np.int32), data_len=np.diff(o.astype(np.int64)).astype(np.int32), use_m=0, names=nb, name_off=noff, ops_stride=64)
    if paired:
        a.update(results=None, first_alt=None, flag=np.zeros(n, np.int32), first_written=np.zeros(2, np.int32))
    if call == "snapgpu_align_sam_paired":
        a.update(contig=np.zeros(n, np.int32), pos=np.zeros(n, np.int64), mapq=np.zeros(n, np.int32), ops=np.zeros(n * 64, np.uint32), n_ops=np.zeros(n, np.int32),
                 nm=np.zeros(n, np.int32), rnext=np.zeros(n, np.int32), pnext=np.zeros(n, np.int64), tlen=np.zeros(n, np.int64),
                 reference_history_dependent=np.zeros(n, np.int32))
    elif call.endswith("_bgzf"):
        a.update(block_input=256, bgzf_capacity=8192, bgzf=np.zeros(8192, np.uint8), member_begin=_words(40), member_capacity=39, n_members=_words(1),
                 bgzf_bytes=_words(1), bam_bytes=_words(1))
    else:
        a.update(text_capacity=8192, text=np.zeros(8192, np.uint8), line_begin=_words((4 if paired else 8) + 1), text_bytes=_words(1))
    return a, key


# ---------------------------------------------------------------------------------------------------------------- the defects
def _decreasing(name):
    def f(a):
        a[name] = a[name].copy(); a[name][1] = a[name][2] + 1
    return f


def _set(**kw):
    return lambda a: a.update(kw)


def _map_out_of_range(a):
    k = "unit_pair" if "unit_pair" in a else "rec_read"
    a[k] = a[k].copy(); a[k][1] = a["n_pairs" if k == "unit_pair" else "n_reads"]


def _null_map(a):                                                            # (rec_read NULL with 6 records of 3 reads; unit_pair NULL with 2 units of 3 pairs)
    a.update({"unit_pair" if "unit_pair" in a else "rec_read": None})
    if "n_pairs" in a:
        a["n_pairs"] = 3


def _no_units(a):
    a.update({k: 0 for k in COUNTS if k in a and not isinstance(a[k], np.ndarray)})


def _no_room(a):
    for cap, buf in (("text_capacity", "text"), ("bgzf_capacity", "bgzf"), ("out_capacity", "out")):
        if cap in a:
            a.update({cap: 0, buf: None})


DEFECTS = {
    "ops_stride=0": _set(ops_stride=0), "ops_stride=2": _set(ops_stride=2), "block_input=0": _set(block_input=0), "block_input=0xff01": _set(block_input=0xff01),
    "offsets decrease": _decreasing("offsets"), "name_off decreases": _decreasing("name_off"), "map out of range": _map_out_of_range, "no map": _null_map,
    "n_units=2^31": _set(n_units=2 ** 31), "n_pairs=2^31": _set(n_pairs=2 ** 31), "n_records=2^32-1": _set(n_records=2 ** 32 - 1), "n_units=2^31-1": _set(n_units=2 ** 31 - 1),
    "record_capacity=2^32-1": _set(record_capacity=2 ** 32 - 1), "n_pairs=2^31-1": _set(n_pairs=2 ** 31 - 1), "blocks=2^32": _set(n_bytes=2 ** 32, block_input=1),
    # the accepted edges
    "n=0": _no_units, "capacity=0": _no_room, "one read, record_capacity=0": _set(n=1, record_capacity=0, flag=None),
}
CONTEXT_DEFECTS = {"no names or numbers": "bare_", "paired context": "paired", "single-end context": "single", "paired context with secondaries": "paired_secondary"}


def defects_of(call):
    """the defects and accepted edges a call is run with (the rows of the table are these, for every call)"""
    names = [n for n, t in signature(call)]
    out = ["null:" + n for n, t in signature(call) if t is None and n not in OPTIONAL]
    host = not call.endswith("_device")
    if call.startswith("snapgpu_bgzf_compress"):
        return out + ["block_input=0", "block_input=0xff01", "blocks=2^32", "block_input=0+null:member_begin", "block_input=0+blocks=2^32", "n=0", "capacity=0"]
    out += ["ops_stride=0", "no names or numbers", "no names or numbers+ops_stride=0", "null:names+ops_stride=0", "n=0", "n=0+ops_stride=0"]
    if call != "snapgpu_align_sam_paired":
        out += ["capacity=0"]
    if is_fused(call):
        out += ["ops_stride=2", "offsets decrease", "ops_stride=2+offsets decrease", "paired context with secondaries"]
        out += ["single-end context", "n_pairs=2^31", "single-end context+ops_stride=2"] if is_paired(call) else ["paired context", "paired context+ops_stride=2"]
        if call != "snapgpu_align_sam_paired":
            out += ["name_off decreases", "offsets decrease+name_off decreases", "n_pairs=2^31-1" if is_paired(call) else "record_capacity=2^32-1"]
            out += ["no names or numbers+" + ("single-end context" if is_paired(call) else "paired context")]
        if "block_input" in names:
            out += ["block_input=0", "block_input=0xff01", "block_input=0+null:bases", "block_input=0+ops_stride=0", "null:n_members+null:bam_bytes"]
        if not is_paired(call):
            out += ["one read, record_capacity=0"]
        return out
    out += ["n_units=2^31", "n_units=2^31-1", "n_units=2^31+ops_stride=0", "n_units=2^31+no names or numbers"] if is_paired(call) else ["n_records=2^32-1", "n_records=2^32-1+ops_stride=0"]
    if host:
        out += ["offsets decrease", "name_off decreases", "map out of range", "no map", "no map+offsets decrease", "offsets decrease+map out of range"]
        if is_paired(call):
            out += ["n_pairs=2^31", "n_pairs=2^31+n_units=2^31"]
    return out


# ---------------------------------------------------------------------------------------------------------------- one row
def run_row(ctxs, hb, call, defect):
    """(return code, message, {output word: value}) of one call.  hb: util.HipBuffers for the device forms' arrays."""
    from snap_amd.aligner import ptr
    a, key = accepted(call, ctxs)
    for d in defect.split("+"):
        if d in CONTEXT_DEFECTS:
            key = CONTEXT_DEFECTS[d] + key if CONTEXT_DEFECTS[d].endswith("_") else CONTEXT_DEFECTS[d]
        elif d.startswith("null:"):
            assert d[5:] in a, (call, d)
            a[d[5:]] = None
        else:
            DEFECTS[d](a)
    if key.startswith("bare_") and "secondary" in key:
        key = "bare_paired"
    ctx = ctxs.get(key)
    sig = signature(call)
    f = getattr(ctx.lib, call)
    f.argtypes = [t or C.c_void_p for n, t in sig]
    f.restype = C.c_int
    device = call.endswith("_device")
    on_device = {}
    args = []
    for n, t in sig:
        v = a[n] if n != "ctx" or a[n] is None else ctx.handle
        if isinstance(v, np.ndarray):
            if device and n not in HOST_WORDS:
                on_device[n] = hb.upload(v)
                v = C.c_void_p(on_device[n])
            else:
                v = ptr(v)
        args.append(v)
    ctx.lib.snapgpu_set_last_error.argtypes = [C.c_char_p]
    ctx.lib.snapgpu_set_last_error(b"")
    try:
        rc = f(*args)
        outs = {}
        for n in HOST_WORDS + OUT_ARRAYS:
            if isinstance(a.get(n), np.ndarray):
                w = int((hb.download(on_device[n], a[n]) if n in on_device else a[n])[0])
                if w != SENT:
                    outs[n] = w
    finally:
        if on_device:
            hb.free_all()
    msg = ctx.lib.snapgpu_last_error(args[0]).decode() if rc < 0 else ""
    return rc, msg, outs


def check_call(ctxs, hb, call, rows):
    """every row of `call`: the return code, the message and the output words are the table's; the rows are those of defects_of(call)"""
    mine = [r for r in rows if r[0] == call]
    assert [r[1] for r in mine] == defects_of(call), call
    bad = []
    for _, defect, rc, msg, outs in mine:
        got = run_row(ctxs, hb, call, defect)
        if got != (rc, msg, outs):
            bad.append((defect, got, (rc, msg, outs)))
    assert not bad, "%s: %d of %d rows differ (defect, got, expected):\n%s" % (call, len(bad), len(mine), "\n".join(map(repr, bad)))
    return len(mine)


# ---------------------------------------------------------------------------------------------------------------- the table
ROWS = [
    ('snapgpu_align_sam_paired', 'null:ctx', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:bases', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:quals', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:offsets', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:front_clip', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:data_len', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:skip', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:flag', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:contig', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:pos', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:mapq', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:ops', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:n_ops', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:nm', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:rnext', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:pnext', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:tlen', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:first_written', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'null:reference_history_dependent', -1, 'snapgpu_align_sam_paired: null argument', {}),
    ('snapgpu_align_sam_paired', 'ops_stride=0', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired', 'no names or numbers', 0, '', {}),
    ('snapgpu_align_sam_paired', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired', 'n=0', 0, '', {}),
    ('snapgpu_align_sam_paired', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired', 'ops_stride=2', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired', 'offsets decrease', -1, 'snapgpu_align_sam_paired: read length out of range', {}),
    ('snapgpu_align_sam_paired', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired', 'paired context with secondaries', -1, 'snapgpu_align_sam_paired: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired', 'single-end context', -1, 'snapgpu_align_sam_paired: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired', 'n_pairs=2^31', -1, 'snapgpu_align_sam_paired: too many pairs', {}),
    ('snapgpu_align_sam_paired', 'single-end context+ops_stride=2', -1, 'snapgpu_align_sam_paired: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'null:ctx', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:bases', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:quals', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:offsets', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:front_clip', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:data_len', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:skip', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:names', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:name_off', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:flag', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:first_written', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:text', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:line_begin', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'null:text_bytes', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'ops_stride=0', -1, 'snapgpu_align_sam_paired_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'no names or numbers', -1, 'snapgpu_align_sam_paired_bam: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_align_sam_paired_bam', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_paired_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_paired_bam: null argument', {}),
    ('snapgpu_align_sam_paired_bam', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_bam', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_paired_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'capacity=0', 3, '', {'text_bytes': 1420, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_bam', 'ops_stride=2', -1, 'snapgpu_align_sam_paired_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'offsets decrease', -1, 'snapgpu_align_sam_paired_bam: read length out of range', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_bam', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_paired_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'paired context with secondaries', -1, 'snapgpu_align_sam_paired_bam: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired_bam', 'single-end context', -1, 'snapgpu_align_sam_paired_bam: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired_bam', 'n_pairs=2^31', -3, 'snapgpu_align_sam_paired_bam: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_align_sam_paired_bam', 'single-end context+ops_stride=2', -1, 'snapgpu_align_sam_paired_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_bam', 'name_off decreases', -1, 'snapgpu_align_sam_paired_bam: name_off must be non-decreasing', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_bam', 'offsets decrease+name_off decreases', -1, 'snapgpu_align_sam_paired_bam: name_off must be non-decreasing', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_bam', 'n_pairs=2^31-1', -3, 'snapgpu_align_sam_paired_bam: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_align_sam_paired_bam', 'no names or numbers+single-end context', -1, 'snapgpu_align_sam_paired_bam: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:ctx', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:bases', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:quals', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:offsets', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:front_clip', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:data_len', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:skip', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:names', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:name_off', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:flag', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:first_written', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:bgzf', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:member_begin', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:n_members', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:bgzf_bytes', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:bam_bytes', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'ops_stride=0', -1, 'snapgpu_align_sam_paired_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'no names or numbers', -1, 'snapgpu_align_sam_paired_bgzf: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_paired_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'n=0', 0, '', {'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_paired_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'capacity=0', 3, '', {'n_members': 6, 'bgzf_bytes': 1351, 'bam_bytes': 1420, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'ops_stride=2', -1, 'snapgpu_align_sam_paired_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'offsets decrease', -1, 'snapgpu_align_sam_paired_bgzf: read length out of range', {'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_paired_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'paired context with secondaries', -1, 'snapgpu_align_sam_paired_bgzf: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'single-end context', -1, 'snapgpu_align_sam_paired_bgzf: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'n_pairs=2^31', -3, 'snapgpu_align_sam_paired_bgzf: more than 2^32 - 1 records in one call', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'single-end context+ops_stride=2', -1, 'snapgpu_align_sam_paired_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'name_off decreases', -1, 'snapgpu_align_sam_paired_bgzf: name_off must be non-decreasing', {'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'offsets decrease+name_off decreases', -1, 'snapgpu_align_sam_paired_bgzf: name_off must be non-decreasing', {'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'n_pairs=2^31-1', -3, 'snapgpu_align_sam_paired_bgzf: more than 2^32 - 1 records in one call', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'no names or numbers+single-end context', -1, 'snapgpu_align_sam_paired_bgzf: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_paired_bgzf', 'block_input=0', -1, 'snapgpu_align_sam_paired_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_paired_bgzf', 'block_input=0xff01', -1, 'snapgpu_align_sam_paired_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_paired_bgzf', 'block_input=0+null:bases', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_bgzf', 'block_input=0+ops_stride=0', -1, 'snapgpu_align_sam_paired_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_paired_bgzf', 'null:n_members+null:bam_bytes', -1, 'snapgpu_align_sam_paired_bgzf: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:ctx', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:bases', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:quals', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:offsets', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:front_clip', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:data_len', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:skip', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:names', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:name_off', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:flag', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:first_written', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:text', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:line_begin', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'null:text_bytes', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'ops_stride=0', -1, 'snapgpu_align_sam_paired_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_text', 'no names or numbers', -1, 'snapgpu_align_sam_paired_text: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_align_sam_paired_text', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_paired_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_text', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_paired_text: null argument', {}),
    ('snapgpu_align_sam_paired_text', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_text', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_paired_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_text', 'capacity=0', 3, '', {'text_bytes': 1720, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_text', 'ops_stride=2', -1, 'snapgpu_align_sam_paired_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_text', 'offsets decrease', -1, 'snapgpu_align_sam_paired_text: read length out of range', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_text', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_paired_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_text', 'paired context with secondaries', -1, 'snapgpu_align_sam_paired_text: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired_text', 'single-end context', -1, 'snapgpu_align_sam_paired_text: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_paired_text', 'n_pairs=2^31', -3, 'snapgpu_align_sam_paired_text: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_align_sam_paired_text', 'single-end context+ops_stride=2', -1, 'snapgpu_align_sam_paired_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_paired_text', 'name_off decreases', -1, 'snapgpu_align_sam_paired_text: name_off must be non-decreasing', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_text', 'offsets decrease+name_off decreases', -1, 'snapgpu_align_sam_paired_text: name_off must be non-decreasing', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_align_sam_paired_text', 'n_pairs=2^31-1', -3, 'snapgpu_align_sam_paired_text: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_align_sam_paired_text', 'no names or numbers+single-end context', -1, 'snapgpu_align_sam_paired_text: a paired-end context without secondary results is needed (snapgpu_enable_paired, no snapgpu_enable_secondary)', {}),
    ('snapgpu_align_sam_single_bam', 'null:ctx', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:bases', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:quals', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:offsets', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:front_clip', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:data_len', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:skip', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:names', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:name_off', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:n_records', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:rec_begin', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:flag', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:text', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:line_begin', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'null:text_bytes', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'ops_stride=0', -1, 'snapgpu_align_sam_single_bam: ops_stride must not be 0', {}),
    ('snapgpu_align_sam_single_bam', 'no names or numbers', -1, 'snapgpu_align_sam_single_bam: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_align_sam_single_bam', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_single_bam: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_align_sam_single_bam', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_single_bam: null argument', {}),
    ('snapgpu_align_sam_single_bam', 'n=0', 0, '', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_bam', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_single_bam: ops_stride must not be 0', {}),
    ('snapgpu_align_sam_single_bam', 'capacity=0', 3, '', {'text_bytes': 720, 'n_records': 3, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_bam', 'ops_stride=2', -1, 'snapgpu_align_sam_single_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_single_bam', 'offsets decrease', -1, 'snapgpu_align_sam_single_bam: read length out of range', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_bam', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_single_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_single_bam', 'paired context with secondaries', -1, 'snapgpu_align_sam_single_bam: a single-end context is needed (no snapgpu_enable_paired)', {}),
    ('snapgpu_align_sam_single_bam', 'paired context', -1, 'snapgpu_align_sam_single_bam: a single-end context is needed (no snapgpu_enable_paired)', {}),
    ('snapgpu_align_sam_single_bam', 'paired context+ops_stride=2', -1, 'snapgpu_align_sam_single_bam: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_single_bam', 'name_off decreases', -1, 'snapgpu_align_sam_single_bam: name_off must be non-decreasing', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_bam', 'offsets decrease+name_off decreases', -1, 'snapgpu_align_sam_single_bam: read length out of range', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_bam', 'record_capacity=2^32-1', -3, 'snapgpu_align_sam_single_bam: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_align_sam_single_bam', 'no names or numbers+paired context', -1, 'snapgpu_align_sam_single_bam: a single-end context is needed (no snapgpu_enable_paired)', {}),
    ('snapgpu_align_sam_single_bam', 'one read, record_capacity=0', 2, '', {'text_bytes': 0, 'n_records': 1, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:ctx', -1, 'snapgpu_align_sam_single_bgzf: null argument', {}),
    ('snapgpu_align_sam_single_bgzf', 'null:bases', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:quals', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:offsets', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:front_clip', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:data_len', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:skip', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:names', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:name_off', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:n_records', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:rec_begin', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:flag', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:bgzf', -1, 'snapgpu_align_sam_single_bgzf: null argument', {}),
    ('snapgpu_align_sam_single_bgzf', 'null:member_begin', -1, 'snapgpu_align_sam_single_bgzf: null argument', {}),
    ('snapgpu_align_sam_single_bgzf', 'null:n_members', -1, 'snapgpu_align_sam_single_bgzf: null argument', {}),
    ('snapgpu_align_sam_single_bgzf', 'null:bgzf_bytes', -1, 'snapgpu_align_sam_single_bgzf: null argument', {}),
    ('snapgpu_align_sam_single_bgzf', 'null:bam_bytes', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'ops_stride=0', -1, 'snapgpu_align_sam_single_bgzf: ops_stride must not be 0', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'no names or numbers', -1, 'snapgpu_align_sam_single_bgzf: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_single_bgzf: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_single_bgzf: null argument', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'n=0', 0, '', {'n_records': 0, 'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'rec_begin': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_single_bgzf: ops_stride must not be 0', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'capacity=0', 3, '', {'n_records': 3, 'n_members': 3, 'bgzf_bytes': 640, 'bam_bytes': 720, 'rec_begin': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'ops_stride=2', -1, 'snapgpu_align_sam_single_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'offsets decrease', -1, 'snapgpu_align_sam_single_bgzf: read length out of range', {'n_records': 0, 'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'rec_begin': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_single_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'paired context with secondaries', -1, 'snapgpu_align_sam_single_bgzf: a single-end context is needed (no snapgpu_enable_paired)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'paired context', -1, 'snapgpu_align_sam_single_bgzf: a single-end context is needed (no snapgpu_enable_paired)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'paired context+ops_stride=2', -1, 'snapgpu_align_sam_single_bgzf: ops_stride must be at least 3', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'name_off decreases', -1, 'snapgpu_align_sam_single_bgzf: name_off must be non-decreasing', {'n_records': 0, 'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'rec_begin': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'offsets decrease+name_off decreases', -1, 'snapgpu_align_sam_single_bgzf: read length out of range', {'n_records': 0, 'n_members': 0, 'bgzf_bytes': 0, 'bam_bytes': 0, 'rec_begin': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'record_capacity=2^32-1', -3, 'snapgpu_align_sam_single_bgzf: more than 2^32 - 1 records in one call', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'no names or numbers+paired context', -1, 'snapgpu_align_sam_single_bgzf: a single-end context is needed (no snapgpu_enable_paired)', {'n_members': 0, 'bgzf_bytes': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_bgzf', 'block_input=0', -1, 'snapgpu_align_sam_single_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_single_bgzf', 'block_input=0xff01', -1, 'snapgpu_align_sam_single_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_single_bgzf', 'block_input=0+null:bases', -1, 'snapgpu_align_sam_single_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_single_bgzf', 'block_input=0+ops_stride=0', -1, 'snapgpu_align_sam_single_bgzf: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_align_sam_single_bgzf', 'null:n_members+null:bam_bytes', -1, 'snapgpu_align_sam_single_bgzf: null argument', {}),
    ('snapgpu_align_sam_single_bgzf', 'one read, record_capacity=0', 2, '', {'n_records': 1, 'n_members': 1, 'bgzf_bytes': 28, 'bam_bytes': 0, 'rec_begin': 0, 'member_begin': 0}),
    ('snapgpu_align_sam_single_text', 'null:ctx', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:bases', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:quals', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:offsets', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:front_clip', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:data_len', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:skip', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:names', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:name_off', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:n_records', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:rec_begin', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:flag', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:text', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:line_begin', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'null:text_bytes', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'ops_stride=0', -1, 'snapgpu_align_sam_single_text: ops_stride must not be 0', {}),
    ('snapgpu_align_sam_single_text', 'no names or numbers', -1, 'snapgpu_align_sam_single_text: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_align_sam_single_text', 'no names or numbers+ops_stride=0', -1, 'snapgpu_align_sam_single_text: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_align_sam_single_text', 'null:names+ops_stride=0', -1, 'snapgpu_align_sam_single_text: null argument', {}),
    ('snapgpu_align_sam_single_text', 'n=0', 0, '', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_text', 'n=0+ops_stride=0', -1, 'snapgpu_align_sam_single_text: ops_stride must not be 0', {}),
    ('snapgpu_align_sam_single_text', 'capacity=0', 3, '', {'text_bytes': 864, 'n_records': 3, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_text', 'ops_stride=2', -1, 'snapgpu_align_sam_single_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_single_text', 'offsets decrease', -1, 'snapgpu_align_sam_single_text: read length out of range', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_text', 'ops_stride=2+offsets decrease', -1, 'snapgpu_align_sam_single_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_single_text', 'paired context with secondaries', -1, 'snapgpu_align_sam_single_text: a single-end context is needed (no snapgpu_enable_paired)', {}),
    ('snapgpu_align_sam_single_text', 'paired context', -1, 'snapgpu_align_sam_single_text: a single-end context is needed (no snapgpu_enable_paired)', {}),
    ('snapgpu_align_sam_single_text', 'paired context+ops_stride=2', -1, 'snapgpu_align_sam_single_text: ops_stride must be at least 3', {}),
    ('snapgpu_align_sam_single_text', 'name_off decreases', -1, 'snapgpu_align_sam_single_text: name_off must be non-decreasing', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_text', 'offsets decrease+name_off decreases', -1, 'snapgpu_align_sam_single_text: read length out of range', {'text_bytes': 0, 'n_records': 0, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_align_sam_single_text', 'record_capacity=2^32-1', -3, 'snapgpu_align_sam_single_text: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_align_sam_single_text', 'no names or numbers+paired context', -1, 'snapgpu_align_sam_single_text: a single-end context is needed (no snapgpu_enable_paired)', {}),
    ('snapgpu_align_sam_single_text', 'one read, record_capacity=0', 2, '', {'text_bytes': 0, 'n_records': 1, 'line_begin': 0, 'rec_begin': 0}),
    ('snapgpu_bam_records_paired', 'null:ctx', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:bases', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:quals', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:offsets', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:names', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:name_off', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:flag', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:contig', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:pos', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:mapq', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:ops', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:n_ops', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:nm', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:rnext', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:pnext', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:tlen', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:first_written', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:text', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:line_begin', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'null:text_bytes', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'ops_stride=0', -1, 'snapgpu_bam_records_paired: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_paired', 'no names or numbers', -1, 'snapgpu_bam_records_paired: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_paired', 'no names or numbers+ops_stride=0', -1, 'snapgpu_bam_records_paired: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_paired', 'null:names+ops_stride=0', -1, 'snapgpu_bam_records_paired: null argument', {}),
    ('snapgpu_bam_records_paired', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_bam_records_paired', 'n=0+ops_stride=0', -1, 'snapgpu_bam_records_paired: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_paired', 'capacity=0', 3, '', {'text_bytes': 745, 'line_begin': 0}),
    ('snapgpu_bam_records_paired', 'n_units=2^31', -3, 'snapgpu_bam_records_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_paired', 'n_units=2^31-1', -3, 'snapgpu_bam_records_paired: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_bam_records_paired', 'n_units=2^31+ops_stride=0', -3, 'snapgpu_bam_records_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_paired', 'n_units=2^31+no names or numbers', -3, 'snapgpu_bam_records_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_paired', 'offsets decrease', -1, 'snapgpu_bam_records_paired: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_bam_records_paired', 'name_off decreases', -1, 'snapgpu_bam_records_paired: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_bam_records_paired', 'map out of range', -1, 'snapgpu_bam_records_paired: unit_pair names a pair the batch does not have', {}),
    ('snapgpu_bam_records_paired', 'no map', -1, 'snapgpu_bam_records_paired: without unit_pair there is one unit per pair (n_units == n_pairs)', {}),
    ('snapgpu_bam_records_paired', 'no map+offsets decrease', -1, 'snapgpu_bam_records_paired: without unit_pair there is one unit per pair (n_units == n_pairs)', {}),
    ('snapgpu_bam_records_paired', 'offsets decrease+map out of range', -1, 'snapgpu_bam_records_paired: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_bam_records_paired', 'n_pairs=2^31', -1, 'snapgpu_bam_records_paired: too many pairs', {}),
    ('snapgpu_bam_records_paired', 'n_pairs=2^31+n_units=2^31', -3, 'snapgpu_bam_records_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_paired_device', 'null:ctx', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:bases', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:quals', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:offsets', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:names', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:name_off', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:flag', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:contig', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:pos', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:mapq', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:ops', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:n_ops', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:nm', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:rnext', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:pnext', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:tlen', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:first_written', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:text', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:line_begin', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'null:text_bytes', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'ops_stride=0', -1, 'snapgpu_bam_records_paired_device: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_paired_device', 'no names or numbers', -1, 'snapgpu_bam_records_paired_device: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_paired_device', 'no names or numbers+ops_stride=0', -1, 'snapgpu_bam_records_paired_device: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_paired_device', 'null:names+ops_stride=0', -1, 'snapgpu_bam_records_paired_device: null argument', {}),
    ('snapgpu_bam_records_paired_device', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_bam_records_paired_device', 'n=0+ops_stride=0', -1, 'snapgpu_bam_records_paired_device: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_paired_device', 'capacity=0', 3, '', {'text_bytes': 745, 'line_begin': 0}),
    ('snapgpu_bam_records_paired_device', 'n_units=2^31', -3, 'snapgpu_bam_records_paired_device: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_paired_device', 'n_units=2^31-1', -3, 'snapgpu_bam_records_paired_device: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_bam_records_paired_device', 'n_units=2^31+ops_stride=0', -3, 'snapgpu_bam_records_paired_device: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_paired_device', 'n_units=2^31+no names or numbers', -3, 'snapgpu_bam_records_paired_device: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_bam_records_single', 'null:ctx', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:bases', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:quals', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:offsets', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:names', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:name_off', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:flag', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:contig', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:pos', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:mapq', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:ops', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:n_ops', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:nm', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:text', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:line_begin', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'null:text_bytes', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'ops_stride=0', -1, 'snapgpu_bam_records_single: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_single', 'no names or numbers', -1, 'snapgpu_bam_records_single: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_single', 'no names or numbers+ops_stride=0', -1, 'snapgpu_bam_records_single: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_single', 'null:names+ops_stride=0', -1, 'snapgpu_bam_records_single: null argument', {}),
    ('snapgpu_bam_records_single', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_bam_records_single', 'n=0+ops_stride=0', -1, 'snapgpu_bam_records_single: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_single', 'capacity=0', 3, '', {'text_bytes': 1328, 'line_begin': 0}),
    ('snapgpu_bam_records_single', 'n_records=2^32-1', -3, 'snapgpu_bam_records_single: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_bam_records_single', 'n_records=2^32-1+ops_stride=0', -1, 'snapgpu_bam_records_single: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_single', 'offsets decrease', -1, 'snapgpu_bam_records_single: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_bam_records_single', 'name_off decreases', -1, 'snapgpu_bam_records_single: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_bam_records_single', 'map out of range', -1, 'snapgpu_bam_records_single: rec_read names a read the batch does not have', {}),
    ('snapgpu_bam_records_single', 'no map', -1, 'snapgpu_bam_records_single: without rec_read there is one record per read (n_records == n_reads)', {}),
    ('snapgpu_bam_records_single', 'no map+offsets decrease', -1, 'snapgpu_bam_records_single: without rec_read there is one record per read (n_records == n_reads)', {}),
    ('snapgpu_bam_records_single', 'offsets decrease+map out of range', -1, 'snapgpu_bam_records_single: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_bam_records_single_device', 'null:ctx', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:bases', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:quals', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:offsets', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:names', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:name_off', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:flag', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:contig', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:pos', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:mapq', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:ops', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:n_ops', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:nm', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:text', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:line_begin', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'null:text_bytes', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'ops_stride=0', -1, 'snapgpu_bam_records_single_device: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_single_device', 'no names or numbers', -1, 'snapgpu_bam_records_single_device: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_single_device', 'no names or numbers+ops_stride=0', -1, 'snapgpu_bam_records_single_device: no contig BAM numbers (call snapgpu_set_contig_bam_ids first)', {}),
    ('snapgpu_bam_records_single_device', 'null:names+ops_stride=0', -1, 'snapgpu_bam_records_single_device: null argument', {}),
    ('snapgpu_bam_records_single_device', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_bam_records_single_device', 'n=0+ops_stride=0', -1, 'snapgpu_bam_records_single_device: ops_stride must not be 0', {}),
    ('snapgpu_bam_records_single_device', 'capacity=0', 3, '', {'text_bytes': 1328, 'line_begin': 0}),
    ('snapgpu_bam_records_single_device', 'n_records=2^32-1', -3, 'snapgpu_bam_records_single_device: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_bam_records_single_device', 'n_records=2^32-1+ops_stride=0', -1, 'snapgpu_bam_records_single_device: ops_stride must not be 0', {}),
    ('snapgpu_bgzf_compress', 'null:ctx', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'null:in', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'null:out', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'null:member_begin', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'null:n_members', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'null:out_bytes', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'block_input=0', -1, 'snapgpu_bgzf_compress: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_bgzf_compress', 'block_input=0xff01', -1, 'snapgpu_bgzf_compress: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_bgzf_compress', 'blocks=2^32', -3, 'snapgpu_bgzf_compress: more than 2^32 - 1 blocks in one call', {}),
    ('snapgpu_bgzf_compress', 'block_input=0+null:member_begin', -1, 'snapgpu_bgzf_compress: null argument', {}),
    ('snapgpu_bgzf_compress', 'block_input=0+blocks=2^32', -3, 'snapgpu_bgzf_compress: more than 2^32 - 1 blocks in one call', {}),
    ('snapgpu_bgzf_compress', 'n=0', 0, '', {'n_members': 1, 'out_bytes': 28, 'member_begin': 0}),
    ('snapgpu_bgzf_compress', 'capacity=0', 3, '', {'n_members': 3, 'out_bytes': 195, 'member_begin': 0}),
    ('snapgpu_bgzf_compress_device', 'null:ctx', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'null:in', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'null:out', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'null:member_begin', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'null:n_members', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'null:out_bytes', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'block_input=0', -1, 'snapgpu_bgzf_compress_device: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_bgzf_compress_device', 'block_input=0xff01', -1, 'snapgpu_bgzf_compress_device: block_input must be between 1 and 0xff00', {}),
    ('snapgpu_bgzf_compress_device', 'blocks=2^32', -3, 'snapgpu_bgzf_compress_device: more than 2^32 - 1 blocks in one call', {}),
    ('snapgpu_bgzf_compress_device', 'block_input=0+null:member_begin', -1, 'snapgpu_bgzf_compress_device: null argument', {}),
    ('snapgpu_bgzf_compress_device', 'block_input=0+blocks=2^32', -3, 'snapgpu_bgzf_compress_device: more than 2^32 - 1 blocks in one call', {}),
    ('snapgpu_bgzf_compress_device', 'n=0', 0, '', {'n_members': 1, 'out_bytes': 28, 'member_begin': 0}),
    ('snapgpu_bgzf_compress_device', 'capacity=0', 3, '', {'n_members': 3, 'out_bytes': 195, 'member_begin': 0}),
    ('snapgpu_sam_text_paired', 'null:ctx', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:bases', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:quals', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:offsets', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:names', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:name_off', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:flag', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:contig', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:pos', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:mapq', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:ops', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:n_ops', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:nm', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:rnext', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:pnext', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:tlen', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:first_written', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:text', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:line_begin', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'null:text_bytes', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'ops_stride=0', -1, 'snapgpu_sam_text_paired: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_paired', 'no names or numbers', -1, 'snapgpu_sam_text_paired: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_paired', 'no names or numbers+ops_stride=0', -1, 'snapgpu_sam_text_paired: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_paired', 'null:names+ops_stride=0', -1, 'snapgpu_sam_text_paired: null argument', {}),
    ('snapgpu_sam_text_paired', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_sam_text_paired', 'n=0+ops_stride=0', -1, 'snapgpu_sam_text_paired: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_paired', 'capacity=0', 3, '', {'text_bytes': 870, 'line_begin': 0}),
    ('snapgpu_sam_text_paired', 'n_units=2^31', -3, 'snapgpu_sam_text_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_paired', 'n_units=2^31-1', -3, 'snapgpu_sam_text_paired: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_sam_text_paired', 'n_units=2^31+ops_stride=0', -3, 'snapgpu_sam_text_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_paired', 'n_units=2^31+no names or numbers', -3, 'snapgpu_sam_text_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_paired', 'offsets decrease', -1, 'snapgpu_sam_text_paired: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_sam_text_paired', 'name_off decreases', -1, 'snapgpu_sam_text_paired: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_sam_text_paired', 'map out of range', -1, 'snapgpu_sam_text_paired: unit_pair names a pair the batch does not have', {}),
    ('snapgpu_sam_text_paired', 'no map', -1, 'snapgpu_sam_text_paired: without unit_pair there is one unit per pair (n_units == n_pairs)', {}),
    ('snapgpu_sam_text_paired', 'no map+offsets decrease', -1, 'snapgpu_sam_text_paired: without unit_pair there is one unit per pair (n_units == n_pairs)', {}),
    ('snapgpu_sam_text_paired', 'offsets decrease+map out of range', -1, 'snapgpu_sam_text_paired: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_sam_text_paired', 'n_pairs=2^31', -1, 'snapgpu_sam_text_paired: too many pairs', {}),
    ('snapgpu_sam_text_paired', 'n_pairs=2^31+n_units=2^31', -3, 'snapgpu_sam_text_paired: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_paired_device', 'null:ctx', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:bases', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:quals', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:offsets', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:names', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:name_off', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:flag', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:contig', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:pos', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:mapq', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:ops', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:n_ops', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:nm', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:rnext', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:pnext', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:tlen', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:first_written', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:text', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:line_begin', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'null:text_bytes', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'ops_stride=0', -1, 'snapgpu_sam_text_paired_device: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_paired_device', 'no names or numbers', -1, 'snapgpu_sam_text_paired_device: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_paired_device', 'no names or numbers+ops_stride=0', -1, 'snapgpu_sam_text_paired_device: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_paired_device', 'null:names+ops_stride=0', -1, 'snapgpu_sam_text_paired_device: null argument', {}),
    ('snapgpu_sam_text_paired_device', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_sam_text_paired_device', 'n=0+ops_stride=0', -1, 'snapgpu_sam_text_paired_device: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_paired_device', 'capacity=0', 3, '', {'text_bytes': 870, 'line_begin': 0}),
    ('snapgpu_sam_text_paired_device', 'n_units=2^31', -3, 'snapgpu_sam_text_paired_device: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_paired_device', 'n_units=2^31-1', -3, 'snapgpu_sam_text_paired_device: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_sam_text_paired_device', 'n_units=2^31+ops_stride=0', -3, 'snapgpu_sam_text_paired_device: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_paired_device', 'n_units=2^31+no names or numbers', -3, 'snapgpu_sam_text_paired_device: more than 2^31 - 1 pair units in one call', {}),
    ('snapgpu_sam_text_single', 'null:ctx', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:bases', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:quals', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:offsets', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:names', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:name_off', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:flag', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:contig', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:pos', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:mapq', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:ops', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:n_ops', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:nm', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:text', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:line_begin', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'null:text_bytes', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'ops_stride=0', -1, 'snapgpu_sam_text_single: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_single', 'no names or numbers', -1, 'snapgpu_sam_text_single: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_single', 'no names or numbers+ops_stride=0', -1, 'snapgpu_sam_text_single: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_single', 'null:names+ops_stride=0', -1, 'snapgpu_sam_text_single: null argument', {}),
    ('snapgpu_sam_text_single', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_sam_text_single', 'n=0+ops_stride=0', -1, 'snapgpu_sam_text_single: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_single', 'capacity=0', 3, '', {'text_bytes': 1459, 'line_begin': 0}),
    ('snapgpu_sam_text_single', 'n_records=2^32-1', -3, 'snapgpu_sam_text_single: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_sam_text_single', 'n_records=2^32-1+ops_stride=0', -1, 'snapgpu_sam_text_single: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_single', 'offsets decrease', -1, 'snapgpu_sam_text_single: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_sam_text_single', 'name_off decreases', -1, 'snapgpu_sam_text_single: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_sam_text_single', 'map out of range', -1, 'snapgpu_sam_text_single: rec_read names a read the batch does not have', {}),
    ('snapgpu_sam_text_single', 'no map', -1, 'snapgpu_sam_text_single: without rec_read there is one record per read (n_records == n_reads)', {}),
    ('snapgpu_sam_text_single', 'no map+offsets decrease', -1, 'snapgpu_sam_text_single: without rec_read there is one record per read (n_records == n_reads)', {}),
    ('snapgpu_sam_text_single', 'offsets decrease+map out of range', -1, 'snapgpu_sam_text_single: offsets and name_off must be non-decreasing', {}),
    ('snapgpu_sam_text_single_device', 'null:ctx', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:bases', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:quals', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:offsets', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:names', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:name_off', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:flag', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:contig', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:pos', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:mapq', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:ops', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:n_ops', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:nm', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:text', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:line_begin', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'null:text_bytes', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'ops_stride=0', -1, 'snapgpu_sam_text_single_device: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_single_device', 'no names or numbers', -1, 'snapgpu_sam_text_single_device: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_single_device', 'no names or numbers+ops_stride=0', -1, 'snapgpu_sam_text_single_device: no contig names (call snapgpu_set_contig_names first)', {}),
    ('snapgpu_sam_text_single_device', 'null:names+ops_stride=0', -1, 'snapgpu_sam_text_single_device: null argument', {}),
    ('snapgpu_sam_text_single_device', 'n=0', 0, '', {'text_bytes': 0, 'line_begin': 0}),
    ('snapgpu_sam_text_single_device', 'n=0+ops_stride=0', -1, 'snapgpu_sam_text_single_device: ops_stride must not be 0', {}),
    ('snapgpu_sam_text_single_device', 'capacity=0', 3, '', {'text_bytes': 1459, 'line_begin': 0}),
    ('snapgpu_sam_text_single_device', 'n_records=2^32-1', -3, 'snapgpu_sam_text_single_device: more than 2^32 - 1 records in one call', {}),
    ('snapgpu_sam_text_single_device', 'n_records=2^32-1+ops_stride=0', -1, 'snapgpu_sam_text_single_device: ops_stride must not be 0', {}),
]


def main(emulated_library=None):
    """print the table that the library answers (see the module's text): libsnapgpu.so on the GPU, or the emulated library at the given path"""
    if emulated_library:
        import snap_amd.aligner as al
        os.environ.setdefault("SNAPGPU_EMU_CUS", "4")
        al._lib, al.LIB_PATH = None, emulated_library
    ctxs = Contexts()
    hb = util.HipBuffers(emu=bool(emulated_library))
    try:
        print("ROWS = [")
        for call in CALLS:
            for defect in defects_of(call):
                rc, msg, outs = run_row(ctxs, hb, call, defect)
                print("    (%r, %r, %d, %r, %r)," % (call, defect, rc, msg, outs))
        print("]")
    finally:
        ctxs.close()


if __name__ == "__main__":
    import sys
    main(*sys.argv[1:2])
