// cigar_args.h -- arguments of the kernels in cigar_k.hip, shared with the host side (snapgpu.hip).
#pragma once
#include "dev_common.h"
#include "../../include/snapgpu.h"

struct AGCParamsPOD { int match, sub, gap_open, gap_ext; };

struct CigarArgs {
    DevIndex ix;
    uint32_t n, RL, ops_stride, use_m;
    const uint8_t *data; const uint64_t *off; const int32_t *len; const int64_t *loc; const int32_t *extra_before;
    uint8_t *scratch;                 // waves * lvc_scratch_bytes()
    uint32_t *work_counter;
    uint32_t *ops; int32_t *n_ops; int32_t *edit_distance; int32_t *add_front_clipping; int64_t *extra_after;
};

struct CigarAGArgs {
    DevIndex ix;
    AGCParamsPOD prm;
    uint32_t n, RL, ops_stride, use_m;
    const uint8_t *data; const uint8_t *quals; const uint64_t *off; const int32_t *len; const int64_t *loc; const int32_t *extra_before;
    const int32_t *score;             // the alignment's edit distance: k of computeGlobalScoreNormalized
    uint8_t *scratch; uint64_t scratch_stride;
    uint32_t *work_counter;
    uint32_t *ops; int32_t *n_ops; int32_t *edit_distance; int32_t *add_front_clipping; int64_t *extra_after; int32_t *tail_ins; int32_t *stale;
};

// The SAM-field kernels (cigar_k.hip: k_sam_fields*, k_samf_dp8*) format items: the reads of a batch, the records of a record list, or the
// 2 * n_pairs mates of a paired batch.  What the three launches share; the outputs, the CIGAR rows and the SamfPre rows are per item.
struct SamFieldsCommon {
    DevIndex ix;
    AGCParamsPOD prm;
    uint32_t RL, ops_stride, use_m, use_affine_gap;
    const uint8_t *bases; const uint8_t *quals; const uint64_t *offsets;       // the reads as they came from the file (unclipped)
    const int32_t *front_clip; const int32_t *data_len;                          // Read::clip's result: bases clipped in front, bases kept
    uint8_t *scratch; uint64_t scratch_stride;                                   // per wave: samf_scratch_layout (cigar_k.hip)
    uint32_t *work_counter;
    int32_t *flag; int32_t *contig; int64_t *pos; int32_t *mapq; uint32_t *ops; int32_t *n_ops; int32_t *nm; int32_t *stale;
    // the banded row loops run ahead of the records, eight items to a wavefront (cigar_ag.h: SamfPre; k_samf_dp8*): items * pre_stride bytes, or NULL
    uint8_t *pre; uint64_t pre_stride; uint32_t *pre_counter;
    uint32_t *pre_valid;                                                         // SamfPre records the pre-pass left valid (snapgpu_debug_samf_pre_valid)
};

struct SamFieldsArgs : SamFieldsCommon {
    uint32_t n;
    const snapgpu_single_result *results;                                        // [n]
};

struct SamFieldsPairedArgs : SamFieldsCommon {                                   // the per-read arrays: [2 * n_pairs], read 0 and read 1 of each pair
    uint32_t n_pairs;
    const snapgpu_paired_result *results;                                        // [n_pairs]
    int32_t *rnext; int64_t *pnext; int64_t *tlen;                               // [2 * n_pairs]
    int32_t *first_written;                                                      // [n_pairs]: which read's record comes first in the file
};

// snapgpu_align_sam_single_records: the records of a batch are a list over its reads (sam_records.h).  Record r belongs to read rec_read[r];
// it is the read's primary (kind 0), its k-th secondary result (kind 1, k = r - rec_begin[read] - 1) or its first-ALT result (kind 2), read
// where the align kernels left them: no per-record copy of a read or of a result exists.
#define SAMREC_CHUNK 1024u          // reads per wavefront tile of the list's scan (sam_records.h)
#define SAMREC_PRIMARY 0
#define SAMREC_SECONDARY 1
#define SAMREC_FIRST_ALT 2
struct SamRecSrc {
    const snapgpu_single_result *primary; const snapgpu_single_result *first_alt;      // [n reads]
    const snapgpu_single_result *secondary; uint32_t sec_stride;                        // [n reads * sec_stride]: the align launch's strided output
    const snapgpu_single_result *sec_ovf; uint32_t ovf_stride;                          // [n_overflow * ovf_stride]: the rerun of the reads that outgrew sec_stride
    const uint32_t *sec_slot;                                                           // [n reads] row of sec_ovf, or 0xFFFFFFFF: the read's row of `secondary`
    const uint64_t *rec_begin; const uint32_t *rec_read; const uint8_t *rec_kind;       // [n reads + 1], [records], [records]
};

// the SAM-field kernels over a record list: n records to format, each reaching its read and its result through src
struct SamFieldsRecArgs : SamFieldsCommon {
    uint32_t n;
    SamRecSrc src;
};

// what the host reads back once the record list is counted
struct SamRecSummary {
    unsigned long long total;         // records the batch has
    uint32_t n_overflow;              // reads with more secondary results than sec_stride
    uint32_t max_secondary;           // the most any of those has
    uint32_t cand_overflow;           // a read outgrew its per-wave candidate list (n_secondary 0xFFFFFFFF)
    uint32_t refused;                 // SAMREC_AE_CLIPPED | SAMREC_RERUN_MISMATCH
};
#define SAMREC_AE_CLIPPED 1u        // -ae: a reader-clipped read reaches the end of its contig (adjust.h's limitation)
#define SAMREC_RERUN_MISMATCH 2u    // the rerun of an overflowed read counted other secondary results than its first pass (cannot happen: the kernels are deterministic)

struct SamRecArgs {
    DevIndex ix;
    uint32_t n, n_chunks, alt_aware, check_clipped, max_k;
    uint64_t cap;                                                                // records the caller has room for
    const uint64_t *offsets; const int32_t *front_clip; const int32_t *data_len;
    const uint32_t *n_secondary;                                                 // [n] or NULL (a context without secondary results)
    uint32_t *count; uint64_t *partial;                                          // [n], [n_chunks]
    uint32_t *sec_slot; uint32_t *ovf_list;                                      // [n] each (ovf_list: the reads to rerun)
    SamRecSummary *summary;
    uint64_t *rec_begin; uint32_t *rec_read; uint8_t *rec_kind;                  // [n + 1], [cap], [cap]: what src's pointers of the same name read
    SamRecSrc src;
    // the rerun's batch: the overflowed reads as a batch of their own (offsets / Read::clip's outcome gathered, the bases stay where they are)
    uint64_t *ovf_offsets; int32_t *ovf_front_clip; int32_t *ovf_data_len;
    const uint32_t *ovf_n_secondary;                                             // [n_overflow] what the rerun counted
    uint64_t *clip_off;                                                          // [n] offsets[i] + front_clip[i]: where the adjuster's read starts
};
// snapgpu_sam_text_single*: records -> the bytes of their SAM lines (sam_text.h).  Record r belongs to read rec_read[r] (NULL: read r).
#define SAMTEXT_NM_OVERFLOW 1u      // a record whose cigar did not fit ops_stride (nm == -2: sam_fields.h)
#define SAMTEXT_BAD_RECORD 2u       // n_ops > ops_stride or a contig the index does not have: printed as "*", the call is refused
                                    // (pair lines: also rnext < -2 or not a contig, first_written outside {0, 1})
struct SamTextSummary {
    unsigned long long total;         // bytes the lines of the batch need
    unsigned long long written;       // end of the last line that lies wholly below the capacity
    uint32_t flags, pad;
};
struct SamTextArgs {
    uint32_t n, n_chunks, ops_stride, n_contigs;                                 // n records, in tiles of SAMREC_CHUNK
    const uint8_t *bases; const uint8_t *quals; const uint64_t *offsets;         // the reads (unclipped: SEQ and QUAL are the whole read)
    const uint8_t *names; const uint64_t *name_off;                              // read i's name: names[name_off[i] .. name_off[i + 1])
    const uint32_t *rec_read;                                                    // [n] or NULL
    const int32_t *flag; const int32_t *contig; const int64_t *pos; const int32_t *mapq; const uint32_t *ops; const int32_t *n_ops; const int32_t *nm;
    const uint8_t *contig_names; const uint32_t *contig_name_off;                // snapgpu_set_contig_names: a blob and n_contigs + 1 offsets
    uint64_t cap;                                                                // bytes `text` has room for
    uint8_t *text; uint64_t *line_begin;                                         // [cap], [n + 1]
    uint32_t *len; uint64_t *partial;                                            // [n] line lengths, [n_chunks] tile sums -> their exclusive scan
    SamTextSummary *summary;
};
extern "C" void snapgpu_launch_sam_text(const SamTextArgs *a, uint32_t scan_blocks, uint32_t write_blocks, hipStream_t s);
// snapgpu_sam_text_paired*: the two lines of each pair unit (one PairedAlignmentResult of a pair).  Line j of a call is position j & 1 of unit
// u = j >> 1: mate v = first_written[u] first, then the other; its fields are at 2 u + v, its read is 2 k + v of pair k = rec_read[u] (here
// the unit's pair; NULL: unit u is pair u).  n is the number of LINES, 2 * n_units, so the scan kernels run over it as they are.
struct SamTextPairedArgs : SamTextArgs {
    const int32_t *rnext; const int64_t *pnext; const int64_t *tlen;             // [n]
    const int32_t *first_written;                                                // [n / 2]
    int32_t *qs;                                                                 // [n] k_samtext_qs: qs[2 u + v] = QS of mate v of unit u's pair, which the OTHER mate's line prints
};
extern "C" void snapgpu_launch_sam_text_paired(const SamTextPairedArgs *a, uint32_t scan_blocks, uint32_t write_blocks, hipStream_t s);
// snapgpu_bam_records_single* / _paired*: records -> the bytes of their BAM records (sam_bam.h).  The arrays of the text calls, single end (the
// pair members NULL) or pair units; `text` is the record bytes, `line_begin` block_begin, len[r] = 4 + block_size.
#define SAMBAM_LONG_NAME 4u         // a QNAME longer than 254 after the cut: the call is refused (summary->pad: ~ the first such record)
struct SamBamArgs : SamTextPairedArgs {
    const int32_t *ref_id;                                                       // [n_contigs] snapgpu_set_contig_bam_ids: the BAM number of each contig
};
extern "C" void snapgpu_launch_sam_bam(const SamBamArgs *a, int paired, uint32_t scan_blocks, uint32_t write_blocks, hipStream_t s);
// snapgpu_bgzf_compress*: bytes -> BGZF blocks (bgzf.h).  Member m covers in[m * block_input, ...) and is first written into slots + m * slot_stride
// (zero beforehand; slot_stride >= block_input + 31, a multiple of 4); a wavefront of the deflate launch keeps its tokens in tok + wave * tok_stride.
#define BGZF_MAX_BLOCK_INPUT 0xff00u
#define BGZF_LDS_WORDS 4800u        // dwords of LDS per wavefront of k_bgzf_deflate
struct BgzfArgs {
    uint64_t n_bytes; uint32_t block_input, n_members;
    const uint8_t *in;
    uint32_t *tok; uint64_t tok_stride;                                          // [deflate waves * tok_stride], tok_stride >= block_input + 1
    uint8_t *slots; uint64_t slot_stride;                                        // [n_members * slot_stride]
    uint32_t *size; uint64_t *partial;                                           // [n_members + 1] member sizes, [tiles of SAMREC_CHUNK] their sums
    uint64_t cap; uint8_t *out; uint64_t *member_begin;                          // [cap], [n_members + 1]
    SamTextSummary *summary;                                                     // total: bytes all members need; written: end of the last member below cap
};
extern "C" void snapgpu_launch_bgzf(const BgzfArgs *a, uint32_t deflate_blocks, uint32_t scan_blocks, uint32_t place_blocks, hipStream_t s);
// snapgpu_bam_sort*: the BAM records of a batch into coordinate order (bam_sort.h).  Record i is bytes[block_begin[i] .. block_begin[i + 1]).
#define BAMSORT_DECREASING 1u       // block_begin[i + 1] < block_begin[i], or a record that ends behind block_begin[n]
#define BAMSORT_SHORT 2u            // a record shorter than 12 bytes: it has no refID and pos words
#define BAMSORT_LONG 4u             // a record of 4 GB or more
struct BamSortSummary {
    uint32_t ones_lo, ones_hi, zeros_lo, zeros_hi;                               // the bits that are 1 in some key, and those that are 0 in some key
    uint32_t flags, first_bad[3];                                                // BAMSORT_*; per flag (DECREASING, SHORT, LONG): ~ the first record that raised it
};
struct BamSortArgs {
    uint32_t n, n_chunks;                                                        // n records, in tiles of SAMREC_CHUNK
    const uint8_t *bytes; const uint64_t *block_begin;                           // [block_begin[n]], [n + 1]
    uint64_t *key; uint32_t *index;                                              // [n] each, the key pass: key[i], index[i] = i
    BamSortSummary *summary;
    const uint32_t *perm;                                                        // [n] sorted: the record at place r
    uint32_t *len; uint64_t *partial;                                            // [n + 1] the sorted records' lengths, [n_chunks] their tile sums
    uint8_t *sorted; uint64_t *sorted_begin;                                     // [block_begin[n]], [n + 1]
    SamTextSummary *scan_summary;                                                // (what sam_text.h's scan kernels fill)
};
extern "C" void snapgpu_launch_bam_sort_keys(const BamSortArgs *a, uint32_t blocks, hipStream_t s);
// one pass over the 6 bits at `shift`: hist [64 * n_tiles], partial [64 * n_tiles / 1024 + 1], total [1]
extern "C" void snapgpu_launch_bam_sort_pass(const uint64_t *keys_in, const uint32_t *vals_in, uint32_t n, uint32_t shift, uint32_t *hist, uint32_t *partial,
                                             uint32_t *total, uint64_t *keys_out, uint32_t *vals_out, uint32_t blocks, hipStream_t s);
extern "C" void snapgpu_launch_bam_sort_gather(const BamSortArgs *a, uint32_t scan_blocks, uint32_t write_blocks, hipStream_t s);
extern "C" void snapgpu_launch_samrec_count(const SamRecArgs *a, uint32_t blocks, hipStream_t s);
extern "C" void snapgpu_launch_samrec_gather(const SamRecArgs *a, uint32_t m, hipStream_t s);
extern "C" void snapgpu_launch_samrec_list(const SamRecArgs *a, uint32_t blocks, hipStream_t s);
extern "C" void snapgpu_launch_samrec_clip_off(const SamRecArgs *a, uint32_t blocks, hipStream_t s);
// the field kernel and the pre-pass of each of the three launches (cigar_k.hip)
void snapgpu_launch_sam_fields(const SamFieldsArgs &a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
void snapgpu_launch_sam_fields(const SamFieldsRecArgs &a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
void snapgpu_launch_sam_fields(const SamFieldsPairedArgs &a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
void snapgpu_launch_samf_dp8(const SamFieldsArgs &a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
void snapgpu_launch_samf_dp8(const SamFieldsRecArgs &a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
void snapgpu_launch_samf_dp8(const SamFieldsPairedArgs &a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
extern "C" size_t snapgpu_samf_dp8_lds_per_wave(uint32_t RL);
extern "C" uint64_t snapgpu_samf_scratch_stride(uint32_t RL);                 // samf_scratch_layout(RL).stride
extern "C" void snapgpu_launch_cigar_ag(const CigarAGArgs *a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
// snapgpu_adjust_alignments: AlignmentAdjuster::AdjustAlignment for a batch of results (adjust.h), one wavefront per result
struct AdjustArgs {
    DevIndex ix;
    uint32_t n, RL;
    const uint8_t *data; const uint64_t *off; const int32_t *len;
    snapgpu_single_result *results;   // in / out: status, direction, location, score -> status, location, score, clipping_for_read_adjustment
    uint8_t *scratch; uint64_t scratch_stride;        // per wave: the read, its reverse complement (RL bytes each), then adjust_scratch_bytes(RL)
    uint32_t *work_counter;
};
extern "C" void snapgpu_launch_adjust_alignments(const AdjustArgs *a, uint32_t blocks, hipStream_t s);
extern "C" void snapgpu_launch_cigar_lv(const CigarArgs *a, uint32_t blocks, size_t lds_bytes, hipStream_t s);
