// snapgpu_sam.cpp -- FASTQ batcher + SAM writer over the C ABI: the host side of
//     snapgpu-sam single <index-dir> <reads.fq> -o <out.sam> [-d maxDist] [-G-] [-=] [-M] [-Cxx] [-ea] [-D n] [-om n [-omax n] [-mpc n]] [-mrl minReadLength]
//                        [-b readsPerBatch] [-gpus n] [-q contextsPerGpu] [-t formatterThreads]
//     snapgpu-sam paired <index-dir> <reads1.fq> <reads2.fq> -o <out.sam> [same options]
// Streams FASTQ records in batches across include/snapgpu.h -- snapgpu_align_sam_single / snapgpu_align_sam_paired (BaseAligner::AlignRead,
// ChimericPairedEndAligner::align) and snapgpu_sam_fields_single / _paired (what SimpleReadWriter::writeReads / writePairs compute before
// they print) -- and prints the records the way the reference does.
//
// Shape (the reference's: SNAPLib/ParallelTask.h:128-138 runs one aligner per thread over a shared read supplier, SingleAligner.cpp:197-330):
//     reader thread  ->  [batches]  ->  GPU feeder threads  ->  [aligned batches]  ->  formatter threads  ->  writer (batch order)
//   * one context per (GPU, feeder thread), `-q` feeders per GPU (default 2): while one feeder's batch is in the kernel the other's is being
//     copied in / out, so H2D, kernel and D2H of consecutive batches overlap on separate streams without a global lock; the feeders of one GPU
//     share its index blobs (snapgpu_create_replica(..., share_index = 1));
//   * `-gpus n` (default: every visible device): the index is read from disk ONCE, into GPU 0, and replicated into the other GPUs' HBM by
//     snapgpu_broadcast_index (RCCL broadcast over xGMI); batches go to whichever feeder is free, reads never cross GPUs;
//   * results are re-ordered by batch number before they are written, so the file is what a single-threaded run writes.
// What is restated here is host-side text handling only:
//   FASTQReader::getReadFromBuffer   SNAPLib/FASTQ.cpp:148-260   (4-line records, '\r' tolerated; plain or gzip input through zlib)
//   Read::clip (ClipBack)            SNAPLib/Read.h:567-620      (the CLI default -C-+: drop the trailing run of '#' qualities)
//   the "useless read" filter        SNAPLib/SingleAligner.cpp:211-232 (dataLength < -mrl or more Ns than -d: written unaligned)
//   SAMFormat::writeHeader           SNAPLib/SAM.cpp:1204-1305   (@HD, default @RG, @PG, one @SQ per contig in ORIGINAL FASTA order, :1291)
//   SAMFormat::writeRead's snprintf  SNAPLib/SAM.cpp:2078-2098   (field order, PG:Z:SNAP, NM:i, default read-group aux)
//   paired: the both-mates-useless rule (PairedAligner.cpp:680-707), the /1 /2 suffix rule (ReadWriter.cpp:392-404), the mate's quality
//   sum QS:i (SAM.cpp:1826-1837) and writePairs' snprintf (:1855-1877); pairing arithmetic is snapgpu_sam_fields_paired's
// No alignment arithmetic happens on the host: without a GPU snapgpu_create_from_directory fails and so does this program.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <queue>
#include <mutex>
#include <string>
#include <thread>
#include <sys/mman.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>
#include <chrono>
#include <vector>
#include <dlfcn.h>
#include <zlib.h>                        // gzread reads plain and gzip-compressed FASTQ alike (the reference takes .gz input too)

#include "../../../include/snapgpu.h"

// The output is written to "<out>.partial" and renamed when it is complete, so that a run that stops half way (an input error, one of the
// unsupported paired -om corners below) never leaves a truncated SAM -- or a BAM without its end-of-file block -- under the name asked for.
static std::string g_partial_path, g_sort_tmp_path;      // what die() removes: the unfinished output, and -so's spill file once it exists
// where the host threads' time goes (SNAPGPU_SAM_VERBOSE=1 prints it): nanoseconds summed over the threads of a kind
static std::atomic<unsigned long long> g_ns_prep(0), g_ns_align(0), g_ns_mid(0), g_ns_samcall(0), g_ns_format(0), g_ns_write(0), g_ns_parse(0);
static std::atomic<unsigned long long> g_ns_wait_in(0), g_ns_wait_out(0), g_ns_wait_writer(0);      // feeders waiting for parsed batches / for room behind them; the writer waiting for the next batch in order
struct StageTimer {
    std::atomic<unsigned long long> &acc; std::chrono::steady_clock::time_point t0;
    explicit StageTimer(std::atomic<unsigned long long> &a) : acc(a), t0(std::chrono::steady_clock::now()) {}
    ~StageTimer() { acc += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
};
struct StageLap {                            // consecutive stages of one thread: lap(acc) adds the time since the previous lap
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(std::atomic<unsigned long long> &acc) { const auto t = std::chrono::steady_clock::now(); acc += (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(t - t0).count(); t0 = t; }
};
static void die(const char *msg, const char *arg = "") {
    fprintf(stderr, "snapgpu-sam: %s%s\n", msg, arg);
    if (!g_partial_path.empty()) remove(g_partial_path.c_str());
    if (!g_sort_tmp_path.empty()) remove(g_sort_tmp_path.c_str());
    exit(1);
}

struct Contig { std::string name; uint64_t begin; bool is_alt; int orig; };

// the contig table of the index directory: names for RNAME / @SQ (Genome.cpp:203-229, 353-403; GenomeIndex.cpp:1879)
static void load_contigs(const std::string &dir, std::vector<Contig> &contigs, uint64_t &n_bases, uint32_t &padding)
{
    FILE *f = fopen((dir + "/GenomeIndex").c_str(), "r");
    if (!f) die("cannot open GenomeIndex in ", dir.c_str());
    unsigned major = 0, minor = 0, n_tables = 0, seed_len = 0, pad = 0; unsigned long long ovf = 0;
    if (fscanf(f, "%u %u %u %llu %u %u", &major, &minor, &n_tables, &ovf, &seed_len, &pad) != 6) die("malformed GenomeIndex header");
    fclose(f);
    padding = pad;
    f = fopen((dir + "/Genome").c_str(), "rb");
    if (!f) die("cannot open Genome in ", dir.c_str());
    char line[8192];
    long long nb = 0; int nc = 0;
    if (!fgets(line, sizeof(line), f) || sscanf(line, "%lld %d", &nb, &nc) != 2) die("malformed Genome header");
    n_bases = (uint64_t)nb;
    for (int i = 0; i < nc; i++) {
        long long begin = 0, pbegin = 0; int cflags = 0, orig = 0, pflags = 0, name_len = 0, cigar_len = 0, consumed = 0;
        if (!fgets(line, sizeof(line), f) ||
            sscanf(line, "%lld %x %d %lld %x %d %d %n", &begin, &cflags, &orig, &pbegin, &pflags, &name_len, &cigar_len, &consumed) < 7)
            die("malformed contig line in Genome");
        Contig c; c.begin = (uint64_t)begin; c.is_alt = (cflags & 1) != 0; c.orig = orig; c.name.assign(line + consumed, (size_t)name_len);
        contigs.push_back(c);
    }
    fclose(f);
}

// ---------------------------------------------------------------------------------------- FASTQ input
struct LineReader {                      // lines out of a gz / plain file through one large buffer (gzgets is several times slower)
    gzFile f = NULL;
    std::vector<char> buf; size_t pos = 0, end = 0; bool eof = false;
    void open(const char *path) { f = gzopen(path, "rb"); if (!f) die("cannot open ", path); gzbuffer(f, 1 << 20); buf.resize(8u << 20); }
    void close() { if (f) gzclose(f); f = NULL; }
    bool fill() {
        if (eof) return false;
        if (pos > 0) { memmove(buf.data(), buf.data() + pos, end - pos); end -= pos; pos = 0; }
        if (end == buf.size()) buf.resize(buf.size() * 2);
        const int n = gzread(f, buf.data() + end, (unsigned)(buf.size() - end));
        if (n < 0) die("read error in FASTQ input");
        if (n == 0) { eof = true; return false; }
        end += (size_t)n;
        return true;
    }
    // next line without its terminator ('\r' tolerated); false at end of file
    bool line(const char *&s, size_t &n) {
        for (;;) {
            const char *nl = (const char *)memchr(buf.data() + pos, '\n', end - pos);
            if (nl) {
                s = buf.data() + pos; n = (size_t)(nl - s); pos += n + 1;
                if (n > 0 && s[n - 1] == '\r') n--;
                return true;
            }
            if (!fill()) {
                if (pos == end) return false;
                s = buf.data() + pos; n = end - pos; pos = end;
                if (n > 0 && s[n - 1] == '\r') n--;
                return true;
            }
        }
    }
};

struct Batch {
    uint64_t seq = 0;
    std::vector<uint32_t> name_off;          // n + 1 offsets into names
    std::string names;
    std::vector<char> bases, quals;          // unclipped, concatenated
    std::vector<uint64_t> offsets;           // n + 1
    size_t n() const { return offsets.size() - 1; }
    void clear() { name_off.assign(1, 0); names.clear(); bases.clear(); quals.clear(); offsets.assign(1, 0); }
};

// one FASTQ record appended to the batch; false at end of file (blank lines between records are skipped)
static bool next_read(LineReader &in, Batch &b, uint32_t max_read_len)
{
    const char *s; size_t n;
    do { if (!in.line(s, n)) return false; } while (n == 0);
    if (s[0] != '@') die("FASTQ record does not start with '@': ", std::string(s, n).c_str());
    const size_t id_at = b.names.size();
    b.names.append(s + 1, n - 1); b.name_off.push_back((uint32_t)b.names.size());
    auto id = [&]() { return std::string(b.names.data() + id_at, b.names.size() - id_at); };      // (only built for an error message)
    if (!in.line(s, n)) die("truncated FASTQ record: ", id().c_str());
    const size_t len = n;
    if (len > max_read_len) die("read longer than max_read_len (400; set SNAPGPU_MAX_READ_LEN, at most 1000): ", id().c_str());
    b.bases.insert(b.bases.end(), s, s + n);
    if (!in.line(s, n)) die("truncated FASTQ record: ", id().c_str());
    if (n == 0 || s[0] != '+') die("FASTQ record without '+' line: ", id().c_str());
    if (!in.line(s, n)) die("truncated FASTQ record: ", id().c_str());
    if (n != len) die("FASTQ sequence and quality lengths differ: ", id().c_str());
    b.quals.insert(b.quals.end(), s, s + n);
    b.offsets.push_back(b.bases.size());
    return true;
}

// ---------------------------------------------------------------------------------------- plain FASTQ, read by many threads
// A plain (not gzip) FASTQ file is mapped and indexed by line count -- one pass, the chunks counted side by side -- so that record r is line
// 4 r and any thread can parse any batch of records on its own (FASTQ.h:67 / ReadSupplierQueue.h:76: the reference's reader hands buffers
// to a queue of supplier threads for the same reason).  A file whose lines do not come in fours (blank lines between records, which the
// sequential reader skips) is read by the sequential reader instead; -seqread forces that reader.
struct MappedFastq {
    const char *p = NULL; size_t n = 0;
    static const size_t CHUNK = 1u << 20;
    std::vector<uint64_t> lines_before;       // lines that start before chunk c (c = 0 .. n_chunks)
    uint64_t n_lines = 0;
    bool open(const char *path) {
        const int fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || st.st_size < 2) { ::close(fd); return false; }
        unsigned char magic[2] = {0, 0};
        if (pread(fd, magic, 2, 0) != 2 || (magic[0] == 0x1f && magic[1] == 0x8b)) { ::close(fd); return false; }      // gzip: the sequential reader
        void *m = mmap(NULL, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
        ::close(fd);
        if (m == MAP_FAILED) return false;
        madvise(m, (size_t)st.st_size, MADV_SEQUENTIAL);
        p = (const char *)m; n = (size_t)st.st_size;
        return true;
    }
    void close() { if (p) munmap((void *)p, n); p = NULL; }
    // count the newlines of every chunk with `threads` threads; false when the lines do not come in fours
    bool index(int threads) {
        const size_t n_chunks = (n + CHUNK - 1) / CHUNK;
        std::vector<uint64_t> cnt(n_chunks, 0);
        std::atomic<size_t> next(0);
        std::vector<std::thread> ts;
        for (int t = 0; t < threads; t++)
            ts.emplace_back([&] {
                for (;;) {
                    const size_t c = next.fetch_add(1);
                    if (c >= n_chunks) break;
                    const char *q = p + c * CHUNK, *e = p + (c + 1 == n_chunks ? n : (c + 1) * CHUNK);
                    uint64_t k = 0;
                    while (q < e) { const char *nl = (const char *)memchr(q, '\n', (size_t)(e - q)); if (!nl) break; k++; q = nl + 1; }
                    cnt[c] = k;
                }
            });
        for (auto &t : ts) t.join();
        lines_before.assign(n_chunks + 1, 0);
        for (size_t c = 0; c < n_chunks; c++) lines_before[c + 1] = lines_before[c] + cnt[c];
        n_lines = lines_before[n_chunks] + (p[n - 1] != '\n' ? 1 : 0);          // (a last line without its newline)
        return n_lines % 4 == 0;
    }
    // byte offset of the start of line L (0-based; L < n_lines)
    size_t line_start(uint64_t L) const {
        if (L == 0) return 0;
        // the chunk in which newline number L (1-based) lies: lines_before[c] < L <= lines_before[c + 1]
        size_t lo = 0, hi = lines_before.size() - 1;
        while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (lines_before[mid] < L) lo = mid; else hi = mid; }
        const char *q = p + lo * CHUNK, *e = p + n;
        uint64_t k = lines_before[lo];
        while (q < e) { const char *nl = (const char *)memchr(q, '\n', (size_t)(e - q)); if (!nl) break; q = nl + 1; if (++k == L) return (size_t)(q - p); }
        return n;
    }
};

// `count` records starting at byte `at` of a mapped file, appended to the batch (every `step`-th slot when two files are interleaved is the
// caller's business: paired batches call this per record).  Returns the byte after the last record.
static inline size_t parse_mapped_record(const MappedFastq &f, size_t at, Batch &b, uint32_t max_read_len)
{
    const char *p = f.p, *e = f.p + f.n;
    auto line = [&](const char *&s, size_t &n) -> bool {
        if (at >= f.n) return false;
        const char *q = p + at;
        const char *nl = (const char *)memchr(q, '\n', (size_t)(e - q));
        s = q; n = nl ? (size_t)(nl - q) : (size_t)(e - q); at += n + (nl ? 1 : 0);
        if (n > 0 && s[n - 1] == '\r') n--;
        return true;
    };
    const char *s; size_t n;
    if (!line(s, n)) die("truncated FASTQ file");
    if (n == 0 || s[0] != '@') die("FASTQ record does not start with '@' (blank lines between records? -seqread reads such files): ", std::string(s, n < 80 ? n : 80).c_str());
    const size_t id_at = b.names.size();
    b.names.append(s + 1, n - 1); b.name_off.push_back((uint32_t)b.names.size());
    auto id = [&]() { return std::string(b.names.data() + id_at, b.names.size() - id_at); };
    if (!line(s, n)) die("truncated FASTQ record: ", id().c_str());
    const size_t len = n;
    if (len > max_read_len) die("read longer than max_read_len (400; set SNAPGPU_MAX_READ_LEN, at most 1000): ", id().c_str());
    b.bases.insert(b.bases.end(), s, s + n);
    if (!line(s, n)) die("truncated FASTQ record: ", id().c_str());
    if (n == 0 || s[0] != '+') die("FASTQ record without '+' line: ", id().c_str());
    if (!line(s, n)) die("truncated FASTQ record: ", id().c_str());
    if (n != len) die("FASTQ sequence and quality lengths differ: ", id().c_str());
    b.quals.insert(b.quals.end(), s, s + n);
    b.offsets.push_back(b.bases.size());
    return at;
}

// ---------------------------------------------------------------------------------------- options, shared state
struct Options {
    bool paired = false;
    snapgpu_params p;
    snapgpu_paired_params pp;
    bool use_m = true;                                                     // AlignerOptions.cpp:58
    unsigned min_read_len = 50;                                            // -mrl
    size_t batch_reads = 0;                                                // -b; 0 = auto (main)
    size_t group = 0;                                                      // -g: single-end batches per GPU call (0 = auto: up to ~1 M reads)
    bool clip_front = false, clip_back = true;                             // -C-+ (ClipBack) is the default
    int om = -1, mpc = -1; long long omax = 0x7fffffff;
    bool ae = false;                                                       // -ae: AlignmentAdjuster before the -om filter (single end only)
    bool stop_on_first_hit = false, explore_popular_seeds = false;         // -f, -x (single end; the paired-end aligners ignore them, as the reference's do)
    int n_gpus = 0, ctx_per_gpu = 0, n_format = 0, n_parse = 0;
    bool seqread = false;                                                  // -seqread: the sequential FASTQ reader even for a plain file
    int passes = 1;                                                        // -passes N (measurement): stream the input N times over the resident index
    uint32_t ops_stride = 64;
    bool bam = false;                                                      // -o x.bam: BAM records in BGZF blocks (SNAPLib/Bam.cpp)
    bool sorted = false; double sort_gb = 16.0;                            // -so: a coordinate-sorted BAM file (sorted runs, merged at the end); -sm: GB of runs held in memory before they spill
    bool verbose = false, host_loop = false;                               // SNAPGPU_SAM_VERBOSE; SNAPGPU_SAM_HOST_LOOP (tests: every record of a multi-result paired batch through the host loop)
    // The path a batch takes, chosen once (choose_paths) from the mode, the output kind, the options and five switches in the environment.
    // Every path writes the same file (BGZF: the same members with other compressed payloads); the opt-in ones are off until they have been
    // timed on a full-size input (DESIGN.md section 13 says what to measure).
    //   `output`, who writes a batch's records     -o x.sam                               -o x.bam
    //   single; paired without -om                 SNAPGPU_SAM_DEVICE_TEXT=1: DeviceText  SNAPGPU_SAM_DEVICE_BGZF=1: DeviceBgzf; else SNAPGPU_SAM_DEVICE_BAM=1: DeviceBam
    //   paired with -om; no switch set             HostFormat                             HostFormat
    //   DeviceText: the batch goes up as it was parsed, with its names, and its SAM lines come down (snapgpu_align_sam_single_text / _paired_text);
    //   DeviceBam: its uncompressed BAM records (.._bam), which the formatter threads only compress; DeviceBgzf: its BGZF blocks (.._bgzf with
    //   block_input 0xff00: a batch is one compression unit, cut where bgzf_append cuts it) -- the header and end-of-file blocks stay with zlib.
    //   A paired batch in which -ea finds a first-ALT pair goes through the host path whatever `output` says.
    //   With HostFormat, who computes the records' fields:
    //   single, no -om / -ae        `single_one_call`: one call per group of batches (snapgpu_align_sam_single); a first-ALT record in the group: batch by batch
    //   single, -om / -ae / -ea     SNAPGPU_SAM_SINGLE_FUSED=1: `single_records_call`, all records from snapgpu_align_sam_single_records; 0 or unset: -ea alone as
    //                               the row above, -om / -ae through separate calls on the clipped reads that prepare_single gathers (`gather_for_aligner`)
    //   paired, no -om              `paired_one_call` (snapgpu_align_sam_paired) unless SNAPGPU_SAM_PAIRED_FUSED=0, a measurement knob (unset: on);
    //                               off, or with a first-ALT pair: snapgpu_align_paired + snapgpu_sam_fields_paired
    //   paired, -om                 snapgpu_align_paired_secondary, then the records of each pair in rounds (PairedBatch::rounds)
    //   -so (BAM only): DeviceBam without a switch where the table has a device path, through the `_bam_sorted` calls, so that a batch comes down as
    //   a sorted run with its keys; every other batch is formatted on the host and sorted by snapgpu_bam_sort (sort_run); no batch is compressed on its own.
    //   `need_bam_ids`: BAM output with either BAM switch (paired -om too): the contexts get the contigs' BAM reference numbers.
    enum Output { HostFormat, DeviceText, DeviceBam, DeviceBgzf };
    struct Paths { Output output = HostFormat; bool single_one_call = false, single_records_call = false, paired_one_call = false, need_bam_ids = false, gather_for_aligner = false; } paths;
};

// the computed fields of a list of SAM records, cigars in rows of ops_stride (a row that was too short: n_ops -1 with nm -2)
struct Records {
    std::vector<int32_t> flag, contig, mapq, n_ops, nm; std::vector<int64_t> pos;
    std::vector<uint32_t> ops; uint32_t ops_stride = 64;
    void assign(size_t n) { flag.assign(n, 0); contig.assign(n, 0); mapq.assign(n, 0); n_ops.assign(n, 0); nm.assign(n, 0); pos.assign(n, 0); }     // (the cigar rows are with_growing_stride's)
    void resize(size_t n) { flag.resize(n); contig.resize(n); mapq.resize(n); n_ops.resize(n); nm.resize(n); pos.resize(n); }
    void clear() { assign(0); ops.clear(); ops_stride = 64; }
    const uint32_t *cigar(size_t i) const { return ops.data() + i * (size_t)ops_stride; }
    uint32_t *cigar(size_t i) { return ops.data() + i * (size_t)ops_stride; }
};

struct Work {                                // a batch on its way through the pipeline
    Batch b;
    // single-end: one entry per RECORD (a read with secondary results appears once per record); paired: one per read
    std::vector<uint32_t> rec_read; std::vector<char> rec_secondary;
    Records rec;
    std::vector<int32_t> rnext, first_written; std::vector<int64_t> pnext, tlen;
    // paired end: what to write, in order.  A "pair unit" is one PairedAlignmentResult of a pair (the primary, a secondary one, the first
    // ALT one): two records, fields at [2u], [2u + 1] of `rec` and of rnext / pnext / tlen, first_written[u].  A "single unit" is one
    // single-end secondary result of a mate (ReadWriter.cpp:508-590): one record, fields in `srec`.
    struct Emit { uint32_t unit; uint8_t single; };
    std::vector<Emit> emit;
    std::vector<uint32_t> pu_pair; std::vector<char> pu_secondary;       // per pair unit: the pair it belongs to, flag 0x100
    std::vector<uint32_t> su_read;                                       // per single unit: the read (2 * pair + mate)
    Records srec;
    // single end: what prepare_single() leaves for the feeder
    bool prepared = false;
    std::vector<int32_t> front_clip, data_len; std::vector<uint32_t> to_align; std::vector<char> ab, aq; std::vector<uint64_t> ao;
    std::vector<uint8_t> skip;               // single end: read i is not given to the aligner (the fused call's argument)
    uint32_t max_len = 0;                    // the longest read of the batch (unclipped): picks the context's read-length class
    std::string text;                        // the formatted records (BAM: BGZF blocks)
    bool text_done = false;                  // the feeder left the SAM lines in `text` (SNAPGPU_SAM_DEVICE_TEXT): nothing for the formatter to do
    std::vector<uint64_t> keys;              // -so: the keys of the records of `text`, which are in key order once sort_done
    bool sort_done = false;
    bool bgzf_done = false;                  // ... and `text` holds the batch's BGZF blocks already (SNAPGPU_SAM_DEVICE_BGZF): nothing to compress either
    bool bam = false;
    unsigned long long mapped = 0;
    // as newly constructed, but every vector keeps its capacity (WorkPool)
    void reset() {
        b.clear(); b.seq = 0;
        rec_read.clear(); rec_secondary.clear(); rec.clear(); srec.clear(); rnext.clear(); first_written.clear(); pnext.clear(); tlen.clear();
        emit.clear(); pu_pair.clear(); pu_secondary.clear(); su_read.clear();
        prepared = false; front_clip.clear(); data_len.clear(); to_align.clear(); ab.clear(); aq.clear(); ao.clear(); skip.clear();
        max_len = 0; text.clear(); text_done = false; bgzf_done = false; bam = false; mapped = 0; keys.clear(); sort_done = false;
    }
};

// Batches are RECYCLED: a batch of 131 072 reads is ~100 MB of vectors (read text, record fields, cigar operations, the formatted records), and allocating
// them anew for every batch meant ~15 GB of fresh pages per 20 M reads -- page faults in the parser / feeder / formatter threads and an munmap per vector
// when the batch was freed, all serialised on the process's address-space lock (freeing on the writer's thread cost half a pass; freeing on a thread of its
// own slowed the feeders' calls by a half instead: profiles/r06g, r06h).  A recycled batch is as newly constructed except for its vectors' capacity.
struct WorkPool {
    std::mutex m; std::vector<Work *> free_list; size_t cap;
    explicit WorkPool(size_t c) : cap(c) {}
    Work *get() { { std::lock_guard<std::mutex> l(m); if (!free_list.empty()) { Work *w = free_list.back(); free_list.pop_back(); return w; } } return new Work(); }
    void put(Work *w) { w->reset(); { std::lock_guard<std::mutex> l(m); if (free_list.size() < cap) { free_list.push_back(w); return; } } delete w; }
    ~WorkPool() { for (Work *w : free_list) delete w; }
};

template <class T> struct Queue {            // bounded multi-producer multi-consumer queue; close() lets consumers drain and stop
    std::mutex m; std::condition_variable not_empty, not_full; std::deque<T> q; size_t cap; bool closed = false;
    explicit Queue(size_t c) : cap(c) {}
    void push(T v) { std::unique_lock<std::mutex> l(m); not_full.wait(l, [&] { return q.size() < cap; }); q.push_back(std::move(v)); not_empty.notify_one(); }
    bool pop(T &v) {
        std::unique_lock<std::mutex> l(m); not_empty.wait(l, [&] { return !q.empty() || closed; });
        if (q.empty()) return false;
        v = std::move(q.front()); q.pop_front(); not_full.notify_one(); return true;
    }
    // up to `want` items: waits for the first; takes what else is there, and waits a little (`grace`) for the rest while producers are alive
    size_t pop_upto(std::vector<T> &out, size_t want, std::chrono::milliseconds grace) {
        std::unique_lock<std::mutex> l(m); not_empty.wait(l, [&] { return !q.empty() || closed; });
        const auto until = std::chrono::steady_clock::now() + grace;
        for (;;) {
            while (!q.empty() && out.size() < want) { out.push_back(std::move(q.front())); q.pop_front(); not_full.notify_one(); }
            if (out.size() >= want || closed || out.empty()) break;
            if (not_empty.wait_until(l, until, [&] { return !q.empty() || closed; }) == false) break;
        }
        return out.size();
    }
    void close() { std::lock_guard<std::mutex> l(m); closed = true; not_empty.notify_all(); }
};

static char complement(char c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }      // COMPLEMENT[], Tables.cpp

static inline void put_uint(std::string &o, unsigned long long v) { char t[24]; int n = 0; do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v); while (n) o.push_back(t[--n]); }
static inline void put_int(std::string &o, long long v) { if (v < 0) { o.push_back('-'); put_uint(o, (unsigned long long)(-(v + 1)) + 1ull); } else put_uint(o, (unsigned long long)v); }

static void fail_rc(snapgpu_ctx *ctx, const char *what, int rc) { fprintf(stderr, "snapgpu-sam: %s failed (%d): %s\n", what, rc, snapgpu_last_error(ctx)); if (!g_sort_tmp_path.empty()) remove(g_sort_tmp_path.c_str()); exit(1); }

// Read::clip and the useless-read test for read i of the batch (Read.h:586-608: back first, then front; SingleAligner.cpp:211-232)
static inline bool clip_read(const Options &o, const Batch &b, size_t i, int32_t &front_clip, int32_t &data_len)
{
    const char *q = b.quals.data() + b.offsets[i], *s = b.bases.data() + b.offsets[i];
    size_t m = (size_t)(b.offsets[i + 1] - b.offsets[i]), fc = 0;
    if (o.clip_back) while (m > 0 && q[m - 1] == '#') m--;
    if (o.clip_front) while (fc < m && q[fc] == '#') fc++;
    m -= fc;
    front_clip = (int32_t)fc; data_len = (int32_t)m;
    unsigned n_count = 0;
    for (size_t j = 0; j < m; j++) n_count += s[fc + j] == 'N';
    return m >= o.min_read_len && n_count <= o.p.max_k;
}

// ---------------------------------------------------------------------------------------- the record loop on the host (rare path)
// SAMFormat::writePairs / writeRead's attempt loop (SAM.cpp:1630-1721, ReadWriter.cpp:228-311 / :508-590) with the Read's clipping state as an
// INPUT: what sam_fields.h does on the device for a record that starts from a fresh Read, done here for the records that do not -- a later
// result of a read whose earlier record left additional back clipping behind (Read.h:547-553).  One snapgpu_compute_cigar_* call per attempt;
// the arithmetic is sam_fields.h's (createSAMLine, computeCigarString, getRefSpanFromCigar, fillMateInfo), line for line.
static const std::vector<Contig> *g_contigs = NULL; static uint64_t g_n_bases = 0; static uint32_t g_padding = 0;
static int h_contig_at(long long loc) { int lo = 0, hi = (int)g_contigs->size() - 1, c = -1; while (lo <= hi) { const int mid = (lo + hi) >> 1; if ((long long)(*g_contigs)[(size_t)mid].begin <= loc) { c = mid; lo = mid + 1; } else hi = mid - 1; } return c; }
static long long h_contig_end(int c) { return c == (int)g_contigs->size() - 1 ? (long long)g_n_bases : (long long)(*g_contigs)[(size_t)c + 1].begin; }
struct HostRec {
    int flag = 0, contig = -1, mapq = 0, n_ops = -1, nm = -1; long long pos = 0;
    long long final_loc = -1; int final_dir = 0, bases_clipped_before = 0, ref_span = 0, data_len = 0;
    std::vector<uint32_t> ops;
    int back_after = 0;                      // the Read's additional back clipping once the record is written
};
struct HostRes { int status, direction, score, mapq, adj, used_ag, bcb, bca, supplementary; long long location; };

static HostRec host_record(const Options &o, snapgpu_ctx *ctx, const char *bases, const char *quals, int U, int F0, int D0, int back0, const HostRes &res, bool paired)
{
    HostRec out; out.back_after = back0;
    int addF = res.adj, addB = back0;
    int status = res.status, direction = res.direction;
    long long location = status == SNAPGPU_NotFound ? -1 : res.location, final_loc = location;
    const bool ag_branch = o.p.use_affine_gap && (res.used_ag != 0 || res.score > 0);
    int cum = 0, n_adj = 0;
    std::vector<char> od((size_t)U), oq((size_t)U);
    int oriented_dir = -1;
    uint32_t stride = 256;
    for (int attempt = 0; attempt < 2 * (int)o.p.max_read_len + 8; attempt++) {
        const int front = F0 + addF, dlen = D0 - addF - addB;
        long long loc = final_loc;
        if (status == SNAPGPU_NotFound) loc = -1;
        const int dir = loc < 0 ? 0 : direction;
        int clipped_len = dlen, bcb, bca;
        if (dir == 1) { bcb = U - clipped_len - front; bca = front; } else { bcb = front; bca = U - clipped_len - bcb; }
        if (ag_branch || paired) { bcb += res.bcb; bca += res.bca; clipped_len -= res.bcb + res.bca; }
        int flag = res.supplementary ? 0x800 : 0, contig = -1, mapq = 0;
        long long pos = 0, extra = 0;
        if (loc >= 0) {
            if (dir == 1) flag |= 0x10;
            contig = h_contig_at(loc);
            if (contig < 0 || loc + dlen > h_contig_end(contig)) {
                contig = contig + 1; if (contig >= (int)g_contigs->size()) contig = (int)g_contigs->size() - 1;
                extra = (long long)(*g_contigs)[(size_t)contig].begin - loc;
            }
            pos = loc + extra - (long long)(*g_contigs)[(size_t)contig].begin + 1;
            mapq = res.mapq < 0 ? 0 : (res.mapq > 70 ? 70 : res.mapq);
        } else flag |= 0x4;
        int afc = 0, nm = -1, n_ops = -1; bool star = true;
        long long clip_before = 0, clip_after = 0;
        std::vector<uint32_t> ops;
        if (ag_branch && !paired && extra != 0) afc = (int)extra;
        else if (loc >= 0) {
            if (oriented_dir != dir) {
                for (int i = 0; i < U; i++) { if (dir == 1) { od[(size_t)(U - 1 - i)] = complement(bases[i]); oq[(size_t)(U - 1 - i)] = quals[i]; } else { od[(size_t)i] = bases[i]; oq[(size_t)i] = quals[i]; } }
                oriented_dir = dir;
            }
            if (clipped_len < 0 || bcb < 0 || bcb + clipped_len > U) die("paired -om / -ea: clipping arithmetic out of range in the host record loop");
            const uint64_t off[2] = {0, (uint64_t)clipped_len};
            const int32_t len = clipped_len, xb = (int32_t)extra, sc = res.score; const int64_t l64 = loc;
            int32_t r_nops = -1, r_ed = -1, r_afc = 0, r_tail = 0, r_hist = 0; int64_t r_xa = 0;
            for (;;) {
                ops.assign(stride, 0);
                int rc = ag_branch
                    ? snapgpu_compute_cigar_ag(ctx, 1, od.data() + bcb, oq.data() + bcb, (uint64_t)clipped_len, off, &len, &l64, &xb, &sc, o.use_m ? 1 : 0, ops.data(), stride, &r_nops, &r_ed, &r_afc, &r_xa, &r_tail, &r_hist)
                    : snapgpu_compute_cigar_lv(ctx, 1, od.data() + bcb, (uint64_t)clipped_len, off, &len, &l64, &xb, o.use_m ? 1 : 0, ops.data(), stride, &r_nops, &r_ed, &r_afc, &r_xa);
                if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_compute_cigar", rc);
                if (r_nops >= 0 || r_ed != -2 || stride >= 4096) break;          // (-2: the ops did not fit the stride)
                stride *= 4;
            }
            n_ops = r_nops; afc = r_afc;
            if (afc == 0 || n_ops < 0) {
                afc = n_ops < 0 ? 0 : afc;
                nm = n_ops < 0 ? 0 : r_ed;
                if (n_ops >= 0 && r_ed >= 0) { star = false; if (ag_branch) bca += r_tail; clip_before = bcb + extra; clip_after = bca + r_xa; }
            }
        }
        if (afc == 0) {
            out.flag = flag; out.contig = loc >= 0 ? contig : -1; out.pos = pos; out.mapq = mapq; out.nm = nm;
            out.final_loc = loc; out.final_dir = dir; out.bases_clipped_before = bcb; out.data_len = dlen; out.back_after = addB;
            if (loc < 0 || star) { out.n_ops = -1; return out; }
            if (clip_before > 0) out.ops.push_back(((uint32_t)clip_before << 4) | 4u);
            out.ops.insert(out.ops.end(), ops.begin(), ops.begin() + n_ops);
            if (clip_after > 0) out.ops.push_back(((uint32_t)clip_after << 4) | 4u);
            out.n_ops = (int)out.ops.size();
            int span = 0;
            for (int i = 0; i < out.n_ops; i++) { const uint32_t code = out.ops[(size_t)i] & 15u; if (i == 0 ? (code != 4u && code != 5u) : (code != 1u)) span += (int)(out.ops[(size_t)i] >> 4); }
            out.ref_span = span;
            return out;
        }
        n_adj++;
        if (paired) {
            const int co = h_contig_at(final_loc), cn = h_contig_at(final_loc + afc);
            if (cn != co || cn < 0 || final_loc + afc > h_contig_end(co) - (long long)g_padding || n_adj > 2 * (int)o.p.max_read_len) { status = SNAPGPU_NotFound; location = -1; direction = 0; final_loc = -1; continue; }
            if (ag_branch) { if (afc < 0) { cum += afc; if (direction == 0) addF = -cum; else addB = -cum; } else final_loc += afc; }
            else { if (afc > 0) { cum += afc; addF = cum; } final_loc += afc; }
            continue;
        }
        const int c_orig = status == SNAPGPU_NotFound ? -1 : h_contig_at(location), c_new = status == SNAPGPU_NotFound ? -1 : h_contig_at(location + afc);
        const int c_lim = ag_branch ? c_new : c_orig;
        bool give_up = c_new < 0 || c_new != c_orig || n_adj > dlen;
        if (!give_up) give_up = final_loc + afc > h_contig_end(c_lim) - (long long)g_padding;
        if (give_up) { status = SNAPGPU_NotFound; location = -1; direction = 0; final_loc = -1; continue; }
        if (ag_branch) { if (afc < 0) { cum += afc; if (direction == 0) addF = -cum; else addB = -cum; } else final_loc = location + afc; }
        else { if (afc > 0) { cum += afc; addF = cum; } final_loc += afc; }
    }
    out.flag = 0x4; out.n_ops = -1; out.nm = -1; out.back_after = addB;
    return out;
}

// SAMFormat::fillMateInfo (SAM.cpp:1308-1421) from the two mates' own records; rnext: -1 "*", -2 "=", otherwise a contig index
static void host_mate_info(const HostRec &me, const HostRec &mate, bool first_in_pair, bool aligned_as_pair, int &flag, int &contig, long long &pos, int &rnext, long long &pnext, long long &tlen)
{
    flag = me.flag | 0x1 | (first_in_pair ? 0x40 : 0x80); contig = me.contig; pos = me.pos; rnext = -1; pnext = 0; tlen = 0;
    auto contig_for_read = [&](long long loc, int data_len, long long *extra) -> int {
        int c = h_contig_at(loc); *extra = 0;
        if (c < 0 || loc + data_len > h_contig_end(c)) { c = c + 1; if (c >= (int)g_contigs->size()) c = (int)g_contigs->size() - 1; *extra = (long long)(*g_contigs)[(size_t)c].begin - loc; }
        return c;
    };
    long long mate_loc = mate.final_loc, mate_extra = 0; bool rnext_eq = false;
    if (mate_loc >= 0) {
        const int mc = contig_for_read(mate_loc, mate.data_len, &mate_extra);
        mate_loc += mate_extra;
        rnext = mc; pnext = mate_loc - (long long)(*g_contigs)[(size_t)mc].begin + 1;
        if (mate.final_dir == 1) flag |= 0x20;
        if (me.final_loc < 0) { contig = mc; rnext_eq = true; pos = pnext; }
    } else { flag |= 0x8; rnext_eq = true; pnext = pos; }
    if (me.final_loc >= 0 && mate.final_loc >= 0) {
        if (aligned_as_pair) flag |= 0x2;
        long long extra = 0;
        const int c = contig_for_read(me.final_loc, me.data_len, &extra);
        const long long loc = me.final_loc + extra;
        const long long my_start = loc - me.bases_clipped_before - extra, my_end = loc + me.ref_span;
        const long long mate_start = mate_loc - mate.bases_clipped_before - mate_extra, mate_end = mate_loc + mate.ref_span;
        contig = c;
        if (my_start < mate_start) { if (me.final_dir == 0) tlen = mate.final_dir == 1 ? mate_end - my_start : mate_start - my_start; else tlen = mate.final_dir == 0 ? mate_start - my_end : mate_end - my_end; }
        else { if (me.final_dir == 1) tlen = mate.final_dir == 0 ? -(my_end - mate_start) : -(my_end - mate_end); else tlen = mate.final_dir == 0 ? -(my_start - mate_start) : -(my_start - mate_end); }
    }
    if (rnext_eq || (rnext >= 0 && rnext == contig)) rnext = -2;
}

// ---------------------------------------------------------------------------------------- GPU stage
// Contexts of one feeder thread, by READ-LENGTH CLASS.  The aligner's answers do not depend on the buffer size it was built for
// (BaseAligner's maxReadSize only sizes its arrays), but the kernel variant does: reads up to 160 bp run the 192-position affine-gap
// variant at six waves per SIMD, up to 256 bp the 256-position one, the command line's maximum (400 by default, as the reference's
// MAX_READ_LENGTH) the 384-position one at four -- which a run of 150 bp reads used to pay for (profiles/r05a: k_align_single<6> was 76 %
// of the GPU time of FASTQ -> SAM).  The class-0 context of every feeder exists from the start; a longer batch makes its feeder create
// the next class over the same resident index (snapgpu_create_replica_with_params), once.
static const uint32_t RL_CLASS[3] = {160, 256, 0};                       // (0: the command line's maximum)
struct FeederCtx {
    snapgpu_ctx *c[3] = {NULL, NULL, NULL};
    snapgpu_ctx *owner = NULL; int device = 0;                             // whose index blobs they share
};
static uint32_t class_len(const Options &o, int k) { return RL_CLASS[k] && RL_CLASS[k] < o.p.max_read_len ? RL_CLASS[k] : o.p.max_read_len; }
static void configure_ctx(const Options &o, snapgpu_ctx *c)
{
    snapgpu_set_aligner_flags(c, o.stop_on_first_hit ? 1 : 0, o.explore_popular_seeds ? 1 : 0);      // -f, -x (single-end launches only)
    {   // RNAME of the SAM-line kernels (snapgpu_align_sam_single_text): the contig table in the index's order
        std::vector<const char *> names; for (const Contig &ct : *g_contigs) names.push_back(ct.name.c_str());
        int rc = snapgpu_set_contig_names(c, (uint32_t)names.size(), names.data());
        if (rc != SNAPGPU_OK) fail_rc(c, "snapgpu_set_contig_names", rc);
    }
    if (o.paths.need_bam_ids) {   // refID of the BAM-record kernels: the contigs' original numbers, which order the header's reference table (main checks that they are a permutation)
        std::vector<int32_t> ids; for (const Contig &ct : *g_contigs) ids.push_back(ct.orig);
        int rc = snapgpu_set_contig_bam_ids(c, (uint32_t)ids.size(), ids.data());
        if (rc != SNAPGPU_OK) fail_rc(c, "snapgpu_set_contig_bam_ids", rc);
    }
    if (o.paired) { int rc = snapgpu_enable_paired(c, &o.pp); if (rc != SNAPGPU_OK) fail_rc(c, "snapgpu_enable_paired", rc); }
    if (o.om >= 0) {
        snapgpu_secondary_params sp; memset(&sp, 0, sizeof(sp));
        sp.max_edit_distance = o.om; sp.max_per_contig = o.mpc; sp.max_results = o.omax; sp.adjust_alignments = o.ae ? 1u : 0u;
        int rc = snapgpu_enable_secondary(c, &sp);
        if (rc != SNAPGPU_OK) fail_rc(c, "snapgpu_enable_secondary", rc);
    }
}
static snapgpu_ctx *ctx_for(const Options &o, FeederCtx &f, uint32_t max_len)
{
    int k = 0;
    while (k < 2 && max_len > class_len(o, k)) k++;
    while (k < 2 && class_len(o, k) == class_len(o, k + 1) && f.c[k] == NULL) k++;     // (classes that coincide: use the one that exists)
    if (f.c[k]) return f.c[k];
    for (int j = 0; j < 3; j++) if (f.c[j] && class_len(o, j) == class_len(o, k)) return f.c[k] = f.c[j];
    snapgpu_params p = o.p; p.max_read_len = class_len(o, k);
    int rc = snapgpu_create_replica_with_params(f.owner, f.device, 1, &p, &f.c[k]);
    if (rc != SNAPGPU_OK) fail_rc(f.owner, "snapgpu_create_replica_with_params", rc);
    configure_ctx(o, f.c[k]);
    return f.c[k];
}
// the switches of Options::Paths, read once (an unset switch: `unset`; otherwise on unless it reads as 0)
static bool env_switch(const char *name, bool unset) { const char *e = getenv(name); return e ? atoi(e) != 0 : unset; }
static void choose_paths(Options &o)
{
    Options::Paths &p = o.paths;
    const bool text = env_switch("SNAPGPU_SAM_DEVICE_TEXT", false), bgzf = env_switch("SNAPGPU_SAM_DEVICE_BGZF", false), bam = env_switch("SNAPGPU_SAM_DEVICE_BAM", false) || bgzf || o.sorted;
    if (!(o.paired && o.om >= 0)) p.output = o.bam ? (bgzf && !o.sorted ? Options::DeviceBgzf : bam ? Options::DeviceBam : Options::HostFormat) : (text ? Options::DeviceText : Options::HostFormat);
    p.need_bam_ids = o.bam && bam;
    p.single_records_call = !o.paired && env_switch("SNAPGPU_SAM_SINGLE_FUSED", false) && (o.om >= 0 || o.ae || o.p.emit_alt_alignments != 0);
    p.paired_one_call = o.paired && o.om < 0 && env_switch("SNAPGPU_SAM_PAIRED_FUSED", true);
    p.single_one_call = !o.paired && o.om < 0 && !o.ae && !p.single_records_call;
    p.gather_for_aligner = !o.paired && !p.single_one_call && !p.single_records_call && p.output == Options::HostFormat;
    o.verbose = getenv("SNAPGPU_SAM_VERBOSE") != NULL; o.host_loop = getenv("SNAPGPU_SAM_HOST_LOOP") != NULL;
}
// A cigar that does not fit ops_stride comes back as n_ops = -1 with nm = -2 (the reference's "cigarBuf too small" never happens: its
// buffer is large): call again with a larger stride rather than print a wrong record.
static bool cigar_overflowed(const int32_t *nm, size_t n) { for (size_t i = 0; i < n; i++) if (nm[i] == -2) return true; return false; }
static void grow_stride(uint32_t &stride) { if (stride >= 4096) die("a cigar needs more than 4096 operations"); stride *= 4; }
template <class F> static void with_growing_stride(Records &r, size_t n_rec, F call)
{
    for (;;) {
        r.ops.assign(n_rec * (size_t)r.ops_stride, 0);
        call();
        if (!cigar_overflowed(r.nm.data(), n_rec)) return;
        grow_stride(r.ops_stride);
    }
}
static std::atomic<unsigned long long> g_bam_batches(0), g_bam_records(0);      // what the device-BAM paths produced (the line on stderr at the end)
static std::atomic<unsigned long long> g_bgzf_batches(0), g_bgzf_members(0), g_bgzf_in(0), g_bgzf_out(0);      // what SNAPGPU_SAM_DEVICE_BGZF produced (its line on stderr)
static std::atomic<uint32_t> g_bgzf_per_mille(500);             // BGZF capacity of the next call, in thousandths of the record-byte estimate: grows to what batches have needed
static std::atomic<uint32_t> g_text_extra_per_record(128);      // text capacity of the next call: bytes per record beyond its name, SEQ and QUAL; grows to what batches have needed
static std::atomic<uint32_t> g_records_per_read_x16(24);        // record capacity of the next call, in sixteenths of a record per read: grows to what batches have needed
static void raise_to(std::atomic<uint32_t> &a, uint32_t need) { uint32_t cur = a.load(); while (need > cur && !a.compare_exchange_weak(cur, need)) {} }
static size_t record_capacity(size_t n_reads) { return (n_reads * (size_t)g_records_per_read_x16.load() + 15) / 16 + 16; }
static void records_needed(size_t n_rec, size_t n_reads) { raise_to(g_records_per_read_x16, (uint32_t)((n_rec * 16 + n_reads - 1) / n_reads) + 2); }
// Read::clip and the useless-read filter for a batch, and the reads to align gathered into one buffer: host work that does not need the GPU,
// done by the parser threads where there are several (the feeder threads' time belongs to the device)
static void prepare_single(const Options &o, Work &w)
{
    const Batch &b = w.b;
    const size_t n = b.n();
    w.front_clip.assign(n, 0); w.data_len.assign(n, 0); w.skip.assign(n, 1); w.to_align.clear(); w.ab.clear(); w.aq.clear(); w.ao.assign(1, 0);
    const bool gather = o.paths.gather_for_aligner;      // (the one-call paths work on the batch itself: nothing to gather)
    if (gather) { w.ab.reserve(b.bases.size()); w.aq.reserve(b.quals.size()); w.ao.reserve(n + 1); }
    w.to_align.reserve(n);
    w.max_len = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t U = (uint32_t)(b.offsets[i + 1] - b.offsets[i]);
        if (U > w.max_len) w.max_len = U;
        if (clip_read(o, b, i, w.front_clip[i], w.data_len[i])) {
            w.to_align.push_back((uint32_t)i); w.skip[i] = 0;
            if (!gather) continue;
            const char *q = b.quals.data() + b.offsets[i] + w.front_clip[i], *s = b.bases.data() + b.offsets[i] + w.front_clip[i];
            w.ab.insert(w.ab.end(), s, s + w.data_len[i]); w.aq.insert(w.aq.end(), q, q + w.data_len[i]); w.ao.push_back(w.ab.size());
        }
    }
    w.prepared = true;
}
static bool g_index_has_alt = false;        // the index has ALT contigs: only then can a first-ALT result (an extra record) exist
// The adjuster (-ae) is restated for reads the reader has not clipped (adjust.h): the reference settles a contig-end overhang on the
// UNCLIPPED buffer (AlignmentAdjuster.cpp:167), which only differs for a clipped read that hangs over the end of its contig.  Such a
// read is refused rather than answered differently (-C-- switches the reader's clipping off): by the library in its one-call paths
// (SNAPGPU_E_UNSUPPORTED, "-ae: ..."), by refuse_ae_at_contig_end after the separate calls.
static const char AE_REFUSAL[] = "-ae: a quality-clipped read hangs over the end of its contig, which the adjuster does not reproduce (run with -C--)";
static void die_if_ae_refused(const Options &o, snapgpu_ctx *ctx, int rc)
{
    if (rc == SNAPGPU_E_UNSUPPORTED && o.ae && !strncmp(snapgpu_last_error(ctx), "-ae:", 4)) die(AE_REFUSAL);
}
// Options::DeviceText / DeviceBam / DeviceBgzf: the batch goes up as it was parsed, with its names, and its SAM lines (BAM output: its
// uncompressed BAM records, which are shorter than the lines, so the same estimate has room for them; or their BGZF blocks) come down into
// w.text, the records' flags into w.rec.flag.  The capacities start from estimates and follow what the library reports; a cigar that
// outgrows its row is met with a larger row, as with_growing_stride does.  `call(DeviceCall &)` makes the ABI call `<stem>_text`, `_bam` or
// `_bgzf`.  `rec_cap` is the first record capacity or, with `fixed_records` (pairs), the record count itself, which the call does not report.
// `discard()` is asked once the call has succeeded: true sends the batch through the host path after all (false is returned, w.text is empty).
struct DeviceCall {                          // one attempt: the capacities the call is given (`begin`: line_begin or, DeviceBgzf, member_begin) and what it reports
    uint32_t ops_stride; uint64_t rec_cap, text_cap, bgzf_cap, *begin, max_members;
    uint64_t n_rec, text_bytes, n_members, bgzf_bytes;
};
// a batch whose blocks came from the device: the counts of the line on stderr, and the next batch's capacity (est: this batch's record-byte estimate)
static void bgzf_from_device(Work &w, size_t est, uint64_t n_members, uint64_t in_bytes, uint64_t out_bytes)
{
    w.bgzf_done = true;
    g_bgzf_batches++; g_bgzf_members += n_members; g_bgzf_in += in_bytes; g_bgzf_out += out_bytes;
    raise_to(g_bgzf_per_mille, (uint32_t)(out_bytes * 1000 / (est ? est : 1)) + 20);
}
template <class Call, class Discard>
static bool device_output(const Options &o, snapgpu_ctx *ctx, Work &w, const char *stem, size_t rec_cap, bool fixed_records, Call call, Discard discard)
{
    const Batch &b = w.b;
    const size_t n = b.n();
    const bool bgzf = o.paths.output == Options::DeviceBgzf;
    const size_t per_read = (2 * b.bases.size() + b.names.size() + n - 1) / n;             // name, SEQ and QUAL of the average record (pairs: both readers make n even, a record per read)
    size_t cap = rec_cap, tcap = cap * (per_read + g_text_extra_per_record.load());
    size_t zcap = tcap / 1000 * g_bgzf_per_mille.load() + 64;
    std::vector<uint64_t> begin;
    DeviceCall c; memset(&c, 0, sizeof(c));
    c.ops_stride = o.ops_stride;
    for (;;) {
        w.rec.flag.resize(cap); begin.resize(bgzf ? tcap / 0xff00 + 2 : cap + 1); w.text.resize(bgzf ? zcap : tcap);
        if (fixed_records) c.n_rec = cap;
        c.rec_cap = cap; c.text_cap = tcap; c.bgzf_cap = zcap; c.begin = begin.data(); c.max_members = begin.size() - 1;
        const int rc = call(c);
        die_if_ae_refused(o, ctx, rc);
        if (rc == SNAPGPU_W_RECORDS_TRUNCATED) { cap = (size_t)c.n_rec + (size_t)c.n_rec / 16; tcap = cap * (per_read + g_text_extra_per_record.load()); continue; }
        if (rc == SNAPGPU_W_TEXT_TRUNCATED) { tcap = (size_t)c.text_bytes + (size_t)c.text_bytes / 64; if (c.bgzf_bytes > zcap) zcap = (size_t)c.bgzf_bytes + (size_t)c.bgzf_bytes / 64; continue; }
        if (rc == SNAPGPU_E_INVALID && strstr(snapgpu_last_error(ctx), "ops_stride")) { grow_stride(c.ops_stride); continue; }
        if (rc != SNAPGPU_OK) fail_rc(ctx, (std::string(stem) + (bgzf ? "_bgzf" : o.bam ? "_bam" : "_text")).c_str(), rc);
        break;
    }
    if (discard()) { w.text.clear(); w.sort_done = false; return false; }
    const size_t nr = (size_t)c.n_rec;
    if (o.bam) { g_bam_batches++; g_bam_records += nr; }
    if (!fixed_records) records_needed(nr, n);
    if (nr) { const size_t per_rec = ((size_t)c.text_bytes + nr - 1) / nr; raise_to(g_text_extra_per_record, per_rec > per_read ? (uint32_t)(per_rec - per_read) + 16 : 16); }
    w.text.resize((size_t)(bgzf ? c.bgzf_bytes : c.text_bytes)); w.text_done = true; w.mapped = 0;
    if (bgzf) bgzf_from_device(w, tcap, c.n_members, c.text_bytes, c.bgzf_bytes);
    for (size_t r = 0; r < nr; r++) w.mapped += (w.rec.flag[r] & 0x4) == 0;
    return true;
}
static void gpu_single_text(const Options &o, FeederCtx &fc, Work &w)
{
    StageLap lap;
    const Batch &b = w.b;
    const size_t n = b.n();
    w.text.clear(); w.text_done = true; w.mapped = 0;
    if (n == 0) return;
    if (!w.prepared) prepare_single(o, w);
    snapgpu_ctx *ctx = ctx_for(o, fc, w.max_len);
    std::vector<uint64_t> name_off(b.name_off.begin(), b.name_off.end()), rec_begin(n + 1);
    const int use_m = o.use_m ? 1 : 0, adjust_primary = (o.ae && o.om < 0) ? 1 : 0;
    lap(g_ns_prep);
    device_output(o, ctx, w, "snapgpu_align_sam_single", record_capacity(n), false, [&](DeviceCall &c) {
        return o.paths.output == Options::DeviceBgzf
            ? snapgpu_align_sam_single_bgzf(ctx, (uint32_t)n, b.bases.data(), b.quals.data(), b.offsets.data(), w.front_clip.data(), w.data_len.data(),
                                            w.skip.data(), use_m, adjust_primary, b.names.data(), name_off.data(), c.ops_stride,
                                            c.rec_cap, &c.n_rec, rec_begin.data(), w.rec.flag.data(), 0xff00, c.bgzf_cap, (uint8_t *)&w.text[0], c.begin,
                                            c.max_members, &c.n_members, &c.bgzf_bytes, &c.text_bytes)
            : o.sorted
            ? (w.keys.resize((size_t)c.rec_cap), w.sort_done = true,
               snapgpu_align_sam_single_bam_sorted(ctx, (uint32_t)n, b.bases.data(), b.quals.data(), b.offsets.data(), w.front_clip.data(), w.data_len.data(),
                                                   w.skip.data(), use_m, adjust_primary, b.names.data(), name_off.data(), c.ops_stride,
                                                   c.rec_cap, &c.n_rec, rec_begin.data(), w.rec.flag.data(), c.text_cap, (uint8_t *)&w.text[0], c.begin, &c.text_bytes,
                                                   w.keys.data(), NULL))
            : o.paths.output == Options::DeviceBam
            ? snapgpu_align_sam_single_bam(ctx, (uint32_t)n, b.bases.data(), b.quals.data(), b.offsets.data(), w.front_clip.data(), w.data_len.data(),
                                           w.skip.data(), use_m, adjust_primary, b.names.data(), name_off.data(), c.ops_stride,
                                           c.rec_cap, &c.n_rec, rec_begin.data(), w.rec.flag.data(), c.text_cap, (uint8_t *)&w.text[0], c.begin, &c.text_bytes)
            : snapgpu_align_sam_single_text(ctx, (uint32_t)n, b.bases.data(), b.quals.data(), b.offsets.data(), w.front_clip.data(), w.data_len.data(),
                                            w.skip.data(), use_m, adjust_primary, b.names.data(), name_off.data(), c.ops_stride,
                                            c.rec_cap, &c.n_rec, rec_begin.data(), w.rec.flag.data(), c.text_cap, &w.text[0], c.begin, &c.text_bytes);
    }, [] { return false; });
    lap(g_ns_align);
}

// secondary results, -ae, -ea: all records in ONE call -- no clipped copy, no second call for -ae, no results expanded on the host and sent up again
static void single_records_call(const Options &o, snapgpu_ctx *ctx, Work &w, StageLap &lap)
{
    const Batch &b = w.b;
    const size_t n = b.n();
    w.rec.ops_stride = o.ops_stride;
    std::vector<uint64_t> rec_begin(n + 1);
    std::vector<uint8_t> kind;
    std::vector<int32_t> stale;
    uint64_t n_rec = 0;
    size_t cap = record_capacity(n);
    lap(g_ns_prep);
    for (;;) {
        w.rec_read.resize(cap); kind.resize(cap); stale.resize(cap); w.rec.resize(cap);
        w.rec.ops.assign(cap * (size_t)w.rec.ops_stride, 0);
        const int rc = snapgpu_align_sam_single_records(ctx, (uint32_t)n, b.bases.data(), b.quals.data(), b.offsets.data(), w.front_clip.data(), w.data_len.data(),
                                                        w.skip.data(), o.use_m ? 1 : 0, (o.ae && o.om < 0) ? 1 : 0, NULL, NULL, NULL, 0, NULL, (uint64_t)cap, &n_rec,
                                                        rec_begin.data(), w.rec_read.data(), kind.data(), w.rec.flag.data(), w.rec.contig.data(), w.rec.pos.data(), w.rec.mapq.data(),
                                                        w.rec.ops.data(), w.rec.ops_stride, w.rec.n_ops.data(), w.rec.nm.data(), stale.data());
        die_if_ae_refused(o, ctx, rc);
        if (rc == SNAPGPU_W_RECORDS_TRUNCATED) { cap = (size_t)n_rec + (size_t)n_rec / 16; continue; }       // (rare: the capacity follows what batches need)
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_align_sam_single_records", rc);
        if (!cigar_overflowed(w.rec.nm.data(), (size_t)n_rec)) break;
        grow_stride(w.rec.ops_stride);
    }
    const size_t nr = (size_t)n_rec;
    records_needed(nr, n);
    w.rec_read.resize(nr); w.rec.resize(nr); w.rec.ops.resize(nr * (size_t)w.rec.ops_stride);
    w.rec_secondary.resize(nr); for (size_t r = 0; r < nr; r++) w.rec_secondary[r] = kind[r] != 0;      // (0x100 is in the flags already)
    lap(g_ns_align);
}
// the records of a batch as results, in the order they are written: every read's primary, then its secondary results in the aligner's
// order, then its first-ALT result (SingleAligner.cpp:300-322 -> writeReads); w.rec_read / w.rec_secondary beside them
typedef std::vector<snapgpu_single_result> ResultList;
static void add_record(Work &w, ResultList &rec_res, size_t read, bool secondary, const snapgpu_single_result &r) { w.rec_read.push_back((uint32_t)read); w.rec_secondary.push_back(secondary ? 1 : 0); rec_res.push_back(r); }
static snapgpu_single_result not_found_result()                                // SingleAligner.cpp:215-225
{
    snapgpu_single_result r; memset(&r, 0, sizeof(r));
    r.status = SNAPGPU_NotFound; r.location = SNAPGPU_InvalidGenomeLocation32; r.score = -1;
    return r;
}
// the common case in ONE call (snapgpu_align_sam_single): no secondary results, no -ae; one record per read unless a first-ALT result
// turns up.  True when the batch is finished; otherwise (rare) rec_res has the records to compute, ALT ones included, as after the separate calls
static bool single_one_call(const Options &o, snapgpu_ctx *ctx, Work &w, StageLap &lap, ResultList &rec_res)
{
    const Batch &b = w.b;
    const size_t n = b.n();
    const bool want_alt = o.p.alt_awareness && g_index_has_alt;
    ResultList res, alt;
    if (want_alt) { res.resize(n); alt.resize(n); }
    w.rec_read.resize(n); for (size_t i = 0; i < n; i++) w.rec_read[i] = (uint32_t)i;
    w.rec_secondary.assign(n, 0);
    w.rec.assign(n);
    std::vector<int32_t> stale(n);
    w.rec.ops_stride = o.ops_stride;
    lap(g_ns_prep);
    with_growing_stride(w.rec, n, [&] {
        int rc = snapgpu_align_sam_single(ctx, (uint32_t)n, b.bases.data(), b.quals.data(), b.offsets.data(), w.front_clip.data(), w.data_len.data(), w.skip.data(),
                                          o.use_m ? 1 : 0, want_alt ? res.data() : NULL, want_alt ? alt.data() : NULL,
                                          w.rec.flag.data(), w.rec.contig.data(), w.rec.pos.data(), w.rec.mapq.data(), w.rec.ops.data(), w.rec.ops_stride, w.rec.n_ops.data(), w.rec.nm.data(), stale.data());
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_align_sam_single", rc);
    });
    lap(g_ns_align);
    bool any_alt = false;
    if (want_alt) for (size_t i = 0; i < n && !any_alt; i++) any_alt = !w.skip[i] && alt[i].status != SNAPGPU_NotFound;
    if (!any_alt) return true;
    w.rec_read.clear(); w.rec_secondary.clear();
    for (size_t i = 0; i < n; i++) {
        add_record(w, rec_res, i, false, w.skip[i] ? not_found_result() : res[i]);
        if (!w.skip[i] && alt[i].status != SNAPGPU_NotFound) add_record(w, rec_res, i, true, alt[i]);
    }
    return false;
}
static void refuse_ae_at_contig_end(const Options &o, const Work &w, size_t read, const snapgpu_single_result &r)
{
    if (r.status == SNAPGPU_NotFound) return;
    const int c = h_contig_at(r.location);
    if (c >= 0 && r.location + w.data_len[read] + (long long)o.p.max_k + 2 > h_contig_end(c) - (long long)g_padding) die(AE_REFUSAL);
}
// -om / -ae in separate calls: the clipped reads prepare_single gathered go to the aligner and the results are expanded into rec_res
static void single_separate_calls(const Options &o, snapgpu_ctx *ctx, Work &w, StageLap &lap, ResultList &rec_res)
{
    const Batch &b = w.b;
    const size_t n = b.n(), na = w.to_align.size();
    ResultList aligned_res(na), alt_res(na), sec; std::vector<uint32_t> nsec(na, 0);
    uint32_t stride = 0;
    if (na > 0) {
        int rc;
        lap(g_ns_prep);
        if (o.om >= 0) {                     // (-ae with -om: the adjuster runs inside the call, on the primary AND on every secondary result: finalizeSecondaryResults, BaseAligner.cpp:2444-2463)
            stride = 8;
            for (;;) {
                sec.assign(na * stride, snapgpu_single_result());
                rc = snapgpu_align_single_secondary(ctx, (uint32_t)na, w.ab.data(), w.aq.data(), w.ao.data(), aligned_res.data(), alt_res.data(), sec.data(), stride, nsec.data());
                if (rc != SNAPGPU_W_SECONDARY_TRUNCATED) break;
                uint32_t need = stride; for (uint32_t v : nsec) if (v > need) need = v;
                stride = need;
            }
        } else {
            rc = snapgpu_align_single(ctx, (uint32_t)na, w.ab.data(), w.aq.data(), w.ao.data(), aligned_res.data(), alt_res.data());
            if (rc == SNAPGPU_OK && o.ae) {                 // finalizeSecondaryResults has only the primary to adjust (BaseAligner.cpp:2444-2452)
                std::vector<int32_t> lens(na);
                for (size_t k = 0; k < na; k++) lens[k] = (int32_t)(w.ao[k + 1] - w.ao[k]);
                rc = snapgpu_adjust_alignments(ctx, (uint32_t)na, w.ab.data(), (uint64_t)w.ab.size(), w.ao.data(), lens.data(), aligned_res.data());
            }
        }
        for (size_t a = 0; o.ae && rc == SNAPGPU_OK && a < na; a++) {      // every adjusted result: the primary and the nsec[a] secondary ones that are there
            const size_t i = w.to_align[a];
            if (w.front_clip[i] == 0 && (uint64_t)w.data_len[i] == b.offsets[i + 1] - b.offsets[i]) continue;      // the reader clipped nothing
            refuse_ae_at_contig_end(o, w, i, aligned_res[a]);
            for (uint32_t j = 0; j < (nsec[a] < stride ? nsec[a] : stride); j++) refuse_ae_at_contig_end(o, w, i, sec[a * (size_t)stride + j]);
        }
        if (rc != SNAPGPU_OK) fail_rc(ctx, "alignment", rc);
        lap(g_ns_align);
    }
    std::vector<uint32_t> slot(n, 0xffffffffu);
    for (size_t k = 0; k < na; k++) slot[w.to_align[k]] = (uint32_t)k;
    w.rec_read.clear(); w.rec_secondary.clear();
    for (size_t i = 0; i < n; i++) {
        const uint32_t a = slot[i];
        add_record(w, rec_res, i, false, a == 0xffffffffu ? not_found_result() : aligned_res[a]);
        if (a == 0xffffffffu) continue;
        if (o.om >= 0) for (uint32_t j = 0; j < nsec[a]; j++) add_record(w, rec_res, i, true, sec[(size_t)a * stride + j]);
        if (o.p.alt_awareness && alt_res[a].status != SNAPGPU_NotFound) add_record(w, rec_res, i, true, alt_res[a]);      // writeReads(&firstALTResult, 1, firstIsPrimary = false)
    }
}
// whole reads of a batch gathered into a batch of their own (a read appears once per record computed from it), each with the clipping it is given
struct ReadGather { std::vector<char> b, q; std::vector<uint64_t> off = std::vector<uint64_t>(1, 0); std::vector<int32_t> fc, dl; };
static void gather_read(ReadGather &g, const Batch &b, size_t i, int32_t front_clip, int32_t data_len)
{
    g.b.insert(g.b.end(), b.bases.begin() + (long)b.offsets[i], b.bases.begin() + (long)b.offsets[i + 1]);
    g.q.insert(g.q.end(), b.quals.begin() + (long)b.offsets[i], b.quals.begin() + (long)b.offsets[i + 1]);
    g.off.push_back(g.b.size()); g.fc.push_back(front_clip); g.dl.push_back(data_len);
}
// records -> fields: snapgpu_sam_fields_single over rec_res, on the batch itself when every read has one record
static void single_fields_of_records(const Options &o, snapgpu_ctx *ctx, Work &w, StageLap &lap, const ResultList &rec_res)
{
    const Batch &b = w.b;
    const size_t nr = w.rec_read.size();
    const char *bases = b.bases.data(), *quals = b.quals.data(); const uint64_t *off = b.offsets.data(); const int32_t *fc = w.front_clip.data(), *dl = w.data_len.data();
    ReadGather g;
    if (nr != b.n()) {                                                     // (a read with several records: once per record)
        for (size_t r = 0; r < nr; r++) gather_read(g, b, w.rec_read[r], w.front_clip[w.rec_read[r]], w.data_len[w.rec_read[r]]);
        bases = g.b.data(); quals = g.q.data(); off = g.off.data(); fc = g.fc.data(); dl = g.dl.data();
    }
    w.rec.assign(nr);
    std::vector<int32_t> stale(nr);
    w.rec.ops_stride = o.ops_stride;
    lap(g_ns_mid);
    with_growing_stride(w.rec, nr, [&] {
        int rc = snapgpu_sam_fields_single(ctx, (uint32_t)nr, bases, quals, off, fc, dl, rec_res.data(), o.use_m ? 1 : 0,
                                           w.rec.flag.data(), w.rec.contig.data(), w.rec.pos.data(), w.rec.mapq.data(), w.rec.ops.data(), w.rec.ops_stride, w.rec.n_ops.data(), w.rec.nm.data(), stale.data());
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_sam_fields_single", rc);
    });
    lap(g_ns_samcall);
    for (size_t r = 0; r < nr; r++) if (w.rec_secondary[r]) w.rec.flag[r] |= 0x100;                  // SAM_SECONDARY (createSAMLine, SAM.cpp:1477-1479)
}

static void gpu_single(const Options &o, FeederCtx &fc, Work &w)
{
    StageLap lap;
    const size_t n = w.b.n();
    if (!w.prepared) prepare_single(o, w);            // (the parser threads of the mapped reader have done it already)
    snapgpu_ctx *ctx = ctx_for(o, fc, w.max_len);
    if (o.paths.single_records_call && n > 0) { single_records_call(o, ctx, w, lap); return; }
    ResultList rec_res;
    if (o.paths.single_one_call && n > 0) { if (single_one_call(o, ctx, w, lap, rec_res)) return; }
    else single_separate_calls(o, ctx, w, lap, rec_res);
    single_fields_of_records(o, ctx, w, lap, rec_res);
}
// Several batches in ONE GPU call.  The host stages want fine grain -- a batch is parsed by one thread and formatted by one thread, so the
// pipeline fills and drains in the time ONE batch takes -- and the GPU wants ~1 M reads per launch (a launch ends on its slowest read).
// So the batches stay small (131 072 reads) and a feeder hands `-g` of them to snapgpu_align_sam_single as one batch: inputs gathered into
// the feeder's own buffers, outputs scattered back to the batches they belong to, which then go on to the formatters separately.
// Anything but the one-call path (secondary results, -ae, a first-ALT record in the group) is done batch by batch as before.
// The group's buffers are the feeder's own and live as long as it does, so they are worth page-locking: the library takes any host pointer,
// and a pageable one goes through the runtime's staging buffers at a fraction of the link's rate -- ~0.4 GB per call of 1 M reads, up and
// down.  The tool talks to the library through the C ABI only; the HIP runtime the library brought into the process is looked up by name
// (none in the emulator's build of the tool: the buffers then stay pageable).  SNAPGPU_SAM_PIN=0 turns it off.
struct PinnedRange {
    void *p = nullptr; size_t bytes = 0;
    typedef int (*reg_fn)(void *, size_t, unsigned); typedef int (*unreg_fn)(void *);
    static reg_fn reg() { static reg_fn f = (getenv("SNAPGPU_SAM_PIN") && atoi(getenv("SNAPGPU_SAM_PIN")) == 0) ? nullptr : (reg_fn)dlsym(RTLD_DEFAULT, "hipHostRegister"); return f; }
    static unreg_fn unreg() { static unreg_fn f = (unreg_fn)dlsym(RTLD_DEFAULT, "hipHostUnregister"); return f; }
    void release() { if (p && unreg()) (void)unreg()(p); p = nullptr; bytes = 0; }
    // the vector's storage as it is now (after the call's resizes): registered again only when it moved or grew
    template <typename T> void cover(std::vector<T> &v) {
        void *q = (void *)v.data(); const size_t b = v.capacity() * sizeof(T);
        if (q == p && b == bytes) return;
        release();
        static const size_t min_bytes = getenv("SNAPGPU_SAM_PIN_MIN") ? (size_t)atoll(getenv("SNAPGPU_SAM_PIN_MIN")) : ((size_t)1 << 20);
        if (!reg() || !unreg() || b < min_bytes || b == 0) return;
        if (reg()(q, b, 1u /* hipHostRegisterPortable */) == 0) { p = q; bytes = b; }
    }
    ~PinnedRange() { release(); }
};
struct GroupBuf {
    std::vector<char> b, q; std::vector<uint64_t> off; std::vector<int32_t> fc, dl, flag, contig, mapq, n_ops, nm, stale; std::vector<uint8_t> skip;
    std::vector<int64_t> pos; std::vector<uint32_t> ops; std::vector<snapgpu_single_result> res, alt;
    PinnedRange pin[16];
    // resize without ever letting a vector move while its storage is registered: growth releases the registration first (and takes headroom)
    template <typename T> static void fit(std::vector<T> &v, size_t n, PinnedRange &r) { if (n > v.capacity()) { r.release(); v.reserve(n + n / 4); } v.resize(n); }
    void pin_all() {
        pin[0].cover(b); pin[1].cover(q); pin[2].cover(off); pin[3].cover(fc); pin[4].cover(dl); pin[5].cover(flag); pin[6].cover(contig); pin[7].cover(mapq);
        pin[8].cover(n_ops); pin[9].cover(nm); pin[10].cover(stale); pin[11].cover(skip); pin[12].cover(pos); pin[13].cover(ops); pin[14].cover(res); pin[15].cover(alt);
    }
    ~GroupBuf() { for (auto &r : pin) r.release(); }          // (before the vectors go)
};
static void gpu_single_group(const Options &o, FeederCtx &fc, std::vector<Work *> &ws, GroupBuf &g)
{
    if (o.paths.output != Options::HostFormat) { for (Work *w : ws) gpu_single_text(o, fc, *w); return; }
    if (ws.size() == 1 || !o.paths.single_one_call) { for (Work *w : ws) gpu_single(o, fc, *w); return; }
    StageLap lap;
    size_t n = 0, nbytes = 0; uint32_t max_len = 0;
    for (Work *w : ws) { if (!w->prepared) prepare_single(o, *w); n += w->b.n(); nbytes += w->b.bases.size(); if (w->max_len > max_len) max_len = w->max_len; }
    if (n == 0) { for (Work *w : ws) gpu_single(o, fc, *w); return; }
    snapgpu_ctx *ctx = ctx_for(o, fc, max_len);
    GroupBuf::fit(g.b, nbytes, g.pin[0]); GroupBuf::fit(g.q, nbytes, g.pin[1]); GroupBuf::fit(g.off, n + 1, g.pin[2]); GroupBuf::fit(g.fc, n, g.pin[3]);
    GroupBuf::fit(g.dl, n, g.pin[4]); GroupBuf::fit(g.skip, n, g.pin[11]);
    size_t at = 0, ab = 0;
    for (Work *w : ws) {
        const Batch &b = w->b; const size_t m = b.n();
        memcpy(g.b.data() + ab, b.bases.data(), b.bases.size()); memcpy(g.q.data() + ab, b.quals.data(), b.quals.size());
        for (size_t i = 0; i < m; i++) g.off[at + i] = b.offsets[i] + ab;
        memcpy(g.fc.data() + at, w->front_clip.data(), m * 4); memcpy(g.dl.data() + at, w->data_len.data(), m * 4); memcpy(g.skip.data() + at, w->skip.data(), m);
        at += m; ab += b.bases.size();
    }
    g.off[n] = ab;
    const bool want_alt = o.p.alt_awareness && g_index_has_alt;
    if (want_alt) { GroupBuf::fit(g.res, n, g.pin[14]); GroupBuf::fit(g.alt, n, g.pin[15]); }
    GroupBuf::fit(g.flag, n, g.pin[5]); GroupBuf::fit(g.contig, n, g.pin[6]); GroupBuf::fit(g.mapq, n, g.pin[7]); GroupBuf::fit(g.n_ops, n, g.pin[8]);
    GroupBuf::fit(g.nm, n, g.pin[9]); GroupBuf::fit(g.stale, n, g.pin[10]); GroupBuf::fit(g.pos, n, g.pin[12]);
    uint32_t stride = o.ops_stride;
    lap(g_ns_prep);
    for (;;) {
        GroupBuf::fit(g.ops, 0, g.pin[13]); GroupBuf::fit(g.ops, n * (size_t)stride, g.pin[13]);      // (zero-filled: resize from empty)
        g.pin_all();
        const int rc = snapgpu_align_sam_single(ctx, (uint32_t)n, g.b.data(), g.q.data(), g.off.data(), g.fc.data(), g.dl.data(), g.skip.data(), o.use_m ? 1 : 0,
                                                want_alt ? g.res.data() : NULL, want_alt ? g.alt.data() : NULL,
                                                g.flag.data(), g.contig.data(), g.pos.data(), g.mapq.data(), g.ops.data(), stride, g.n_ops.data(), g.nm.data(), g.stale.data());
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_align_sam_single", rc);
        if (!cigar_overflowed(g.nm.data(), n)) break;
        grow_stride(stride);
    }
    lap(g_ns_align);
    if (want_alt) for (size_t i = 0; i < n; i++) if (!g.skip[i] && g.alt[i].status != SNAPGPU_NotFound) { for (Work *w : ws) gpu_single(o, fc, *w); return; }   // (rare: ALT records: batch by batch)
    at = 0;
    for (Work *w : ws) {
        const size_t m = w->b.n();
        Records &r = w->rec;
        w->rec_read.resize(m); for (size_t i = 0; i < m; i++) w->rec_read[i] = (uint32_t)i;
        w->rec_secondary.assign(m, 0);
        auto part = [&](auto &to, const auto &from, size_t per) { to.assign(from.begin() + (long)(at * per), from.begin() + (long)((at + m) * per)); };
        part(r.flag, g.flag, 1); part(r.contig, g.contig, 1); part(r.mapq, g.mapq, 1); part(r.n_ops, g.n_ops, 1); part(r.nm, g.nm, 1); part(r.pos, g.pos, 1);
        r.ops_stride = stride; part(r.ops, g.ops, stride);
        at += m;
    }
    lap(g_ns_mid);
}

typedef std::vector<snapgpu_paired_result> PairedResultList;
static HostRes host_res(const snapgpu_single_result &r)
{
    return HostRes{r.status, r.direction, r.score, r.mapq, r.clipping_for_read_adjustment, r.used_affine_gap_scoring, r.bases_clipped_before, r.bases_clipped_after, r.supplementary, (long long)r.location};
}
static HostRes host_res(const snapgpu_paired_result &r, int v)
{
    return HostRes{r.status[v], r.direction[v], r.score[v], r.mapq[v], r.clipping_for_read_adjustment[v], r.used_affine_gap_scoring[v], r.bases_clipped_before[v], r.bases_clipped_after[v],
                   r.supplementary[v], (long long)r.location[v]};
}
// the pair fields of a batch beside w.rec: sized for n_units pair units and n_singles single units, cigar rows of the starting stride
static void size_pair_fields(const Options &o, Work &w, size_t n_units, size_t n_singles)
{
    const size_t nrec = 2 * n_units;
    w.rec.assign(nrec); w.rnext.assign(nrec, 0); w.first_written.assign(n_units, 0); w.pnext.assign(nrec, 0); w.tlen.assign(nrec, 0);
    w.srec.assign(n_singles);
    w.rec.ops_stride = w.srec.ops_stride = o.ops_stride;
}
// one record's fields and cigar row into place (`from` has the same stride); a record the host loop computed: false when its cigar does not fit the row
static void copy_record(Records &to, size_t dst, const Records &from, size_t src, int or_flag)
{
    to.flag[dst] = from.flag[src] | or_flag; to.contig[dst] = from.contig[src]; to.pos[dst] = from.pos[src]; to.mapq[dst] = from.mapq[src]; to.n_ops[dst] = from.n_ops[src]; to.nm[dst] = from.nm[src];
    memcpy(to.cigar(dst), from.cigar(src), (size_t)to.ops_stride * 4);
}
static bool store_host_record(Records &to, size_t dst, const HostRec &rec, int flag, int contig, long long pos)
{
    if ((uint32_t)(rec.n_ops > 0 ? rec.n_ops : 0) > to.ops_stride) return false;
    to.flag[dst] = flag; to.contig[dst] = contig; to.pos[dst] = pos; to.mapq[dst] = rec.mapq; to.n_ops[dst] = rec.n_ops; to.nm[dst] = rec.nm;
    for (int c = 0; c < rec.n_ops; c++) to.cigar(dst)[c] = rec.ops[(size_t)c];
    return true;
}
// A batch of pairs in its feeder, and gpu_paired's steps over it: one_call; align_calls, emit_list and then one snapgpu_sam_fields_paired call or rounds()
struct PairedBatch {
    const Options &o; snapgpu_ctx *ctx; Work &w; const Batch &b;
    size_t n, np;                            // reads, pairs
    std::vector<int32_t> front_clip, data_len; std::vector<char> useful;      // per read: Read::clip, and whether the aligner gets the read
    PairedBatch(const Options &o_, snapgpu_ctx *c, Work &w_) : o(o_), ctx(c), w(w_), b(w_.b), n(b.n()), np(n / 2), front_clip(n, 0), data_len(n, 0), useful(n, 0)
    {
        for (size_t i = 0; i < n; i++) useful[i] = clip_read(o, b, i, front_clip[i], data_len[i]);
    }
    // The common case in ONE call: no secondary results, one record pair per pair unless -ea has a first-ALT result to write.  The batch goes up
    // as it was parsed and its fields (snapgpu_align_sam_paired) or, on the device-output paths, its lines, records or blocks come down.  True when
    // the batch is finished; false (rare) when it has a first-ALT pair to write and goes through the separate calls: the call was then for nothing.
    bool one_call()
    {
        const size_t nrec = 2 * np;
        const bool want_alt = o.p.emit_alt_alignments != 0;
        const int use_m = o.use_m ? 1 : 0;
        std::vector<uint8_t> skip(np);
        for (size_t k = 0; k < np; k++) skip[k] = !useful[2 * k] && !useful[2 * k + 1];      // neither mate useful (PairedAligner.cpp:680-682)
        PairedResultList fres, falt;
        if (want_alt) { fres.resize(np); falt.resize(np); }
        snapgpu_paired_result *res = want_alt ? fres.data() : NULL, *alt = want_alt ? falt.data() : NULL;
        auto first_alt_pair = [&] {
            if (want_alt) for (size_t k = 0; k < np; k++) if (!skip[k] && (falt[k].status[0] != SNAPGPU_NotFound || falt[k].status[1] != SNAPGPU_NotFound)) return true;
            return false;
        };
        if (o.paths.output != Options::HostFormat) {
            std::vector<uint64_t> name_off(b.name_off.begin(), b.name_off.end());
            w.rec.flag.assign(nrec, 0); w.first_written.assign(np, 0);
            return device_output(o, ctx, w, "snapgpu_align_sam_paired", nrec, true, [&](DeviceCall &c) {
                return o.paths.output == Options::DeviceBgzf
                    ? snapgpu_align_sam_paired_bgzf(ctx, (uint32_t)np, b.bases.data(), b.quals.data(), b.offsets.data(), front_clip.data(), data_len.data(),
                                                    skip.data(), use_m, b.names.data(), name_off.data(), c.ops_stride, res, alt, w.rec.flag.data(), w.first_written.data(),
                                                    0xff00, c.bgzf_cap, (uint8_t *)&w.text[0], c.begin, c.max_members, &c.n_members, &c.bgzf_bytes, &c.text_bytes)
                    : o.sorted
                    ? (w.keys.resize(nrec), w.sort_done = true,
                       snapgpu_align_sam_paired_bam_sorted(ctx, (uint32_t)np, b.bases.data(), b.quals.data(), b.offsets.data(), front_clip.data(), data_len.data(),
                                                           skip.data(), use_m, b.names.data(), name_off.data(), c.ops_stride, res, alt, w.rec.flag.data(), w.first_written.data(),
                                                           c.text_cap, (uint8_t *)&w.text[0], c.begin, &c.text_bytes, w.keys.data(), NULL))
                    : o.paths.output == Options::DeviceBam
                    ? snapgpu_align_sam_paired_bam(ctx, (uint32_t)np, b.bases.data(), b.quals.data(), b.offsets.data(), front_clip.data(), data_len.data(),
                                                   skip.data(), use_m, b.names.data(), name_off.data(), c.ops_stride, res, alt, w.rec.flag.data(), w.first_written.data(),
                                                   c.text_cap, (uint8_t *)&w.text[0], c.begin, &c.text_bytes)
                    : snapgpu_align_sam_paired_text(ctx, (uint32_t)np, b.bases.data(), b.quals.data(), b.offsets.data(), front_clip.data(), data_len.data(),
                                                    skip.data(), use_m, b.names.data(), name_off.data(), c.ops_stride, res, alt, w.rec.flag.data(), w.first_written.data(),
                                                    c.text_cap, &w.text[0], c.begin, &c.text_bytes);
            }, first_alt_pair);
        }
        w.emit.clear(); w.pu_pair.resize(np); w.pu_secondary.assign(np, 0); w.su_read.clear();
        for (size_t k = 0; k < np; k++) { w.emit.push_back(Work::Emit{(uint32_t)k, 0}); w.pu_pair[k] = (uint32_t)k; }
        size_pair_fields(o, w, np, 0);
        std::vector<int32_t> stale(nrec);
        with_growing_stride(w.rec, nrec, [&] {
            int rc = snapgpu_align_sam_paired(ctx, (uint32_t)np, b.bases.data(), b.quals.data(), b.offsets.data(), front_clip.data(), data_len.data(), skip.data(),
                                              use_m, res, alt, w.rec.flag.data(), w.rec.contig.data(), w.rec.pos.data(), w.rec.mapq.data(), w.rec.ops.data(), w.rec.ops_stride, w.rec.n_ops.data(),
                                              w.rec.nm.data(), w.rnext.data(), w.pnext.data(), w.tlen.data(), w.first_written.data(), stale.data());
            if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_align_sam_paired", rc);
        });
        return !first_alt_pair();
    }
    // The separate align calls: the pairs with at least one useful mate (PairedAligner.cpp:680-682), clipped, through snapgpu_align_paired or --
    // secondary results (-om): paired ones and each mate's single-end ones (PairedAligner.cpp:727-779) -- snapgpu_align_paired_secondary
    std::vector<uint32_t> slot;                                          // per pair: its place among the aligned pairs, or NONE
    static constexpr uint32_t NONE = 0xffffffffu;
    PairedResultList results, first_alt;                                       // per pair (NotFound where it was not aligned); per aligned pair: its first-ALT result
    PairedResultList sec; std::vector<uint32_t> nsec; uint32_t sec_stride = 0;            // per aligned pair: further pair results
    ResultList ssec; std::vector<uint32_t> nssec; uint32_t ssec_stride = 0;               // per aligned pair: mate 0's single-end secondary results, then mate 1's (nssec[2 a + v] of them)
    void align_calls()
    {
        std::vector<uint32_t> to_align;
        std::vector<char> ab, aq; std::vector<uint64_t> ao(1, 0);
        slot.assign(np, NONE);
        for (size_t k = 0; k < np; k++) {
            if (!useful[2 * k] && !useful[2 * k + 1]) continue;
            slot[k] = (uint32_t)to_align.size(); to_align.push_back((uint32_t)k);
            for (size_t i = 2 * k; i < 2 * k + 2; i++) {
                const char *q = b.quals.data() + b.offsets[i], *s = b.bases.data() + b.offsets[i];
                ab.insert(ab.end(), s + front_clip[i], s + front_clip[i] + data_len[i]); aq.insert(aq.end(), q + front_clip[i], q + front_clip[i] + data_len[i]); ao.push_back(ab.size());
            }
        }
        const size_t na = to_align.size();
        PairedResultList ares(na);
        snapgpu_paired_result none; memset(&none, 0, sizeof(none));
        for (int v = 0; v < 2; v++) { none.status[v] = SNAPGPU_NotFound; none.location[v] = SNAPGPU_InvalidGenomeLocation32; none.score[v] = -1; }
        results.assign(np, none); first_alt.resize(na); nsec.assign(na, 0); nssec.assign(2 * na, 0);
        if (na == 0) return;
        int rc;
        if (o.om >= 0) {
            sec_stride = 8; ssec_stride = 16;
            for (;;) {
                sec.assign(na * (size_t)sec_stride, snapgpu_paired_result()); ssec.assign(na * (size_t)ssec_stride, snapgpu_single_result());
                rc = snapgpu_align_paired_secondary(ctx, (uint32_t)na, ab.data(), aq.data(), ao.data(), ares.data(), first_alt.data(),
                                                    sec.data(), sec_stride, nsec.data(), ssec.data(), ssec_stride, nssec.data());
                if (rc != SNAPGPU_W_SECONDARY_TRUNCATED) break;
                for (size_t k = 0; k < na; k++) {
                    if (nsec[k] > sec_stride) sec_stride = nsec[k];
                    if (nssec[2 * k] + nssec[2 * k + 1] > ssec_stride) ssec_stride = nssec[2 * k] + nssec[2 * k + 1];
                }
            }
        } else rc = snapgpu_align_paired(ctx, (uint32_t)na, ab.data(), aq.data(), ao.data(), ares.data(), first_alt.data());
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_align_paired", rc);
        for (size_t k = 0; k < na; k++) results[to_align[k]] = ares[k];
    }
    // What gets written, in the reference's order (PairedAligner.cpp:874-880 -> SimpleReadWriter::writePairs): the pair's results (primary first),
    // read 0's single-end secondary results, read 1's, then -- with -ea -- the first ALT result as a pair of its own.  Fills w.emit and its
    // unit tables; pu_res / su_res: the result each pair unit / single unit is computed from
    void emit_list()
    {
        w.emit.clear(); w.pu_pair.clear(); w.pu_secondary.clear(); w.su_read.clear();
        auto add_pair_unit = [&](size_t k, const snapgpu_paired_result &r, bool secondary) {
            w.emit.push_back(Work::Emit{(uint32_t)pu_res.size(), 0}); w.pu_pair.push_back((uint32_t)k); w.pu_secondary.push_back(secondary ? 1 : 0); pu_res.push_back(r);
        };
        for (size_t k = 0; k < np; k++) {
            add_pair_unit(k, results[k], false);
            const uint32_t a = slot[k];
            if (a == NONE) continue;
            if (o.om >= 0) {
                for (uint32_t j = 0; j < nsec[a]; j++) add_pair_unit(k, sec[(size_t)a * sec_stride + j], true);
                uint32_t at = 0;
                for (int v = 0; v < 2; v++) {
                    // (the reference applies the FIRST single result's clippingForReadAdjustment to every one of the mate's single records:
                    //  `singleResults[whichRead]->clippingForReadAdjustment`, ReadWriter.cpp:516)
                    const int32_t first_adj = nssec[2 * a + v] ? ssec[(size_t)a * ssec_stride + at].clipping_for_read_adjustment : 0;
                    for (uint32_t j = 0; j < nssec[2 * a + v]; j++, at++) {
                        snapgpu_single_result r = ssec[(size_t)a * ssec_stride + at];
                        r.clipping_for_read_adjustment = first_adj;
                        w.emit.push_back(Work::Emit{(uint32_t)su_res.size(), 1}); w.su_read.push_back((uint32_t)(2 * k + (size_t)v)); su_res.push_back(r);
                    }
                }
            }
            if (o.p.emit_alt_alignments && (first_alt[a].status[0] != SNAPGPU_NotFound || first_alt[a].status[1] != SNAPGPU_NotFound)) add_pair_unit(k, first_alt[a], false);
        }
    }
    PairedResultList pu_res; ResultList su_res;                          // (emit_list) the result each pair unit / single unit is computed from
    // Several results per pair.  The reference writes them one after the other through the SAME two Read objects, and one piece of their state
    // survives from record to record: the additional BACK clipping that the affine-gap writer sets when it turns a leading insertion of a
    // reverse-complement alignment into a soft clip (SAM.cpp:1676-1680 / ReadWriter.cpp:545-551; setAdditionalFrontClipping is re-set for every
    // result, setAdditionalBackClipping never is: Read.h:537-553).  So the j-th entries of all pairs are computed together (round j), and what a
    // record leaves behind -- readable off its leading soft clip -- shortens the data length the next entry of the same read is given.
    std::vector<std::vector<Work::Emit>> per_pair;                       // per pair: its entries of w.emit, in order
    std::vector<int32_t> carry;                                          // per read: the back clipping its records so far have left
    bool too_small;                                                      // a cigar did not fit its row: the rounds are run again with a larger stride
    bool ag_branch(int used_ag, int score) const { return o.p.use_affine_gap && (used_ag != 0 || score > 0); }
    HostRec on_host(size_t rd, const HostRes &hr, bool paired_rec) const      // (exact: the record loop with the Read's state as it is)
    {
        return host_record(o, ctx, b.bases.data() + b.offsets[rd], b.quals.data() + b.offsets[rd], (int)(b.offsets[rd + 1] - b.offsets[rd]), front_clip[rd], data_len[rd], carry[rd], hr, paired_rec);
    }
    // the state a written record leaves on its Read: `passed_len` is the data length the record was computed with
    // (`hr` / `paired_rec`: the result the record was computed from, for the two cases in which the record alone does not say what it left
    //  behind -- a record given up after clipping adjustments, and a reverse-complement record at the first base of a contig, whose leading
    //  soft clip may have been cut short there: the record loop is then run on the host for that one record, with the Read's state as it
    //  is, and ITS back clipping is what the next record of the read starts from.  Until round 4 these two cases stopped the program.)
    void leave_behind(size_t rd, bool more, bool ag, int status_in, int flag, int64_t pos, int n_ops, const uint32_t *ops, int clipped_before, int passed_len, const HostRes &hr, bool paired_rec)
    {
        if (!more || !ag) return;
        const size_t U = (size_t)(b.offsets[rd + 1] - b.offsets[rd]);
        if (((flag & 0x4) && status_in != SNAPGPU_NotFound) || ((flag & 0x10) && n_ops > 0 && pos == 1)) {
            carry[rd] = on_host(rd, hr, paired_rec).back_after;
            if (o.verbose) fprintf(stderr, "snapgpu-sam: one record's state recomputed on the host (%s), back clipping left: %d\n", (flag & 0x4) ? "given up after clipping adjustments" : "reverse complement at the first base of a contig", carry[rd]);
            return;
        }
        if (!(flag & 0x10) || n_ops <= 0) return;
        const int lead = (ops[0] & 15u) == 4u ? (int)(ops[0] >> 4) : 0;
        const int left = lead - ((int)U - passed_len - front_clip[rd]) - clipped_before;
        if (left < 0) die("internal error: leading soft clip shorter than the read's own clipping");
        if (left > 0) carry[rd] = left;                             // (device-computed records start from carry == 0: the others go through host_record)
    }
    void host_pair_unit(uint32_t u)
    {
        const size_t k = w.pu_pair[u];
        const snapgpu_paired_result &r = pu_res[u];
        HostRec rec[2];
        for (size_t v = 0; v < 2; v++) { rec[v] = on_host(2 * k + v, host_res(r, (int)v), true); carry[2 * k + v] = rec[v].back_after; }
        for (size_t v = 0; v < 2; v++) {
            const size_t dst = 2 * u + v;
            int fl, ct, rn; long long ps, pn, tl;
            host_mate_info(rec[v], rec[1 - v], v == 0, r.aligned_as_pair != 0, fl, ct, ps, rn, pn, tl);
            if (!store_host_record(w.rec, dst, rec[v], fl | (w.pu_secondary[u] ? 0x100 : 0), ct, ps)) { too_small = true; continue; }
            w.rnext[dst] = rn; w.pnext[dst] = pn; w.tlen[dst] = tl;
        }
        const unsigned long long l0 = rec[0].final_loc < 0 ? ~0ull : (unsigned long long)rec[0].final_loc, l1 = rec[1].final_loc < 0 ? ~0ull : (unsigned long long)rec[1].final_loc;
        w.first_written[u] = l0 <= l1 ? 0 : 1;                    // ReadWriter.cpp:481-488
    }
    void device_pair_units(const std::vector<uint32_t> &pus, size_t j)
    {
        const size_t m = pus.size();
        ReadGather g; PairedResultList rr(m);
        for (size_t x = 0; x < m; x++) {
            rr[x] = pu_res[pus[x]];
            for (size_t v = 0; v < 2; v++) { const size_t i = 2 * (size_t)w.pu_pair[pus[x]] + v; gather_read(g, b, i, front_clip[i], data_len[i] - carry[i]); }
        }
        Records t; t.ops_stride = w.rec.ops_stride; t.assign(2 * m); t.ops.resize(2 * m * (size_t)t.ops_stride);
        std::vector<int32_t> rn(2 * m), fw(m), stale(2 * m); std::vector<int64_t> pn(2 * m), tl(2 * m);
        int rc = snapgpu_sam_fields_paired(ctx, (uint32_t)m, g.b.data(), g.q.data(), g.off.data(), g.fc.data(), g.dl.data(), rr.data(), o.use_m ? 1 : 0,
                                           t.flag.data(), t.contig.data(), t.pos.data(), t.mapq.data(), t.ops.data(), t.ops_stride, t.n_ops.data(), t.nm.data(), rn.data(), pn.data(), tl.data(), fw.data(), stale.data());
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_sam_fields_paired", rc);
        if (cigar_overflowed(t.nm.data(), 2 * m)) too_small = true;
        for (size_t x = 0; x < m; x++) {
            const size_t u = pus[x], k = w.pu_pair[u];
            w.first_written[u] = fw[x];
            for (size_t v = 0; v < 2; v++) {
                const size_t src = 2 * x + v, dst = 2 * u + v;
                copy_record(w.rec, dst, t, src, w.pu_secondary[u] ? 0x100 : 0);
                w.rnext[dst] = rn[src]; w.pnext[dst] = pn[src]; w.tlen[dst] = tl[src];
                leave_behind(2 * k + v, j + 1 < per_pair[k].size(), ag_branch(rr[x].used_affine_gap_scoring[v], rr[x].score[v]), rr[x].status[v], t.flag[src], t.pos[src], t.n_ops[src],
                             t.cigar(src), rr[x].bases_clipped_before[v], g.dl[src], host_res(rr[x], (int)v), true);
            }
        }
    }
    void device_single_units(const std::vector<uint32_t> &sus, size_t j)      // records of their own, without mate information (format->writeRead, ReadWriter.cpp:521-527)
    {
        const size_t m = sus.size();
        ReadGather g; ResultList rr(m);
        for (size_t x = 0; x < m; x++) { const size_t i = w.su_read[sus[x]]; rr[x] = su_res[sus[x]]; gather_read(g, b, i, front_clip[i], data_len[i] - carry[i]); }
        Records t; t.ops_stride = w.srec.ops_stride; t.assign(m); t.ops.resize(m * (size_t)t.ops_stride);
        std::vector<int32_t> stale(m);
        int rc = snapgpu_sam_fields_single(ctx, (uint32_t)m, g.b.data(), g.q.data(), g.off.data(), g.fc.data(), g.dl.data(), rr.data(), o.use_m ? 1 : 0,
                                           t.flag.data(), t.contig.data(), t.pos.data(), t.mapq.data(), t.ops.data(), t.ops_stride, t.n_ops.data(), t.nm.data(), stale.data());
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_sam_fields_single", rc);
        if (cigar_overflowed(t.nm.data(), m)) too_small = true;
        for (size_t x = 0; x < m; x++) {
            const size_t r = sus[x], rd = w.su_read[r];
            copy_record(w.srec, r, t, x, 0x100);
            // (a single-end record is written without the aligner's soft clipping unless it went through the affine-gap writer: sam_fields.h)
            const bool ag = ag_branch(rr[x].used_affine_gap_scoring, rr[x].score);
            leave_behind(rd, j + 1 < per_pair[rd / 2].size(), ag, rr[x].status, t.flag[x], t.pos[x], t.n_ops[x], t.cigar(x), ag ? rr[x].bases_clipped_before : 0, g.dl[x], host_res(rr[x]), false);
        }
    }
    void rounds()
    {
        per_pair.assign(np, std::vector<Work::Emit>());
        for (const Work::Emit &e : w.emit) per_pair[e.single ? w.su_read[e.unit] / 2 : w.pu_pair[e.unit]].push_back(e);
        size_t n_rounds = 0;
        for (size_t k = 0; k < np; k++) if (per_pair[k].size() > n_rounds) n_rounds = per_pair[k].size();
        const bool host_all = o.host_loop;
        for (;;) {                                                           // (again with a larger stride when a cigar did not fit)
            too_small = false;
            carry.assign(n, 0);
            w.rec.ops.assign(w.rec.flag.size() * (size_t)w.rec.ops_stride, 0); w.srec.ops.assign(w.srec.flag.size() * (size_t)w.srec.ops_stride, 0);
            for (size_t j = 0; j < n_rounds; j++) {
                std::vector<uint32_t> pus, sus, pus_host, sus_host;          // this round's pair units / single units; `_host`: a read arrives with back clipping
                for (size_t k = 0; k < np; k++) {
                    if (j >= per_pair[k].size()) continue;
                    const Work::Emit &e = per_pair[k][j];
                    if (e.single) (host_all || carry[w.su_read[e.unit]] > 0 ? sus_host : sus).push_back(e.unit);
                    else (host_all || carry[2 * k] > 0 || carry[2 * k + 1] > 0 ? pus_host : pus).push_back(e.unit);
                }
                for (uint32_t u : pus_host) host_pair_unit(u);
                for (uint32_t r : sus_host) {
                    const size_t rd = w.su_read[r];
                    const HostRec rec = on_host(rd, host_res(su_res[r]), false);
                    carry[rd] = rec.back_after;
                    if (!store_host_record(w.srec, r, rec, rec.flag | 0x100, rec.contig, rec.pos)) too_small = true;
                }
                if (!pus.empty()) device_pair_units(pus, j);
                if (!sus.empty()) device_single_units(sus, j);
            }
            if (!too_small) break;
            grow_stride(w.rec.ops_stride); w.srec.ops_stride = w.rec.ops_stride;
        }
    }
};

static void gpu_paired(const Options &o, FeederCtx &fc, Work &w)
{
    const Batch &b = w.b;
    const size_t n = b.n();
    w.max_len = 0;
    for (size_t i = 0; i < n; i++) { const uint32_t U = (uint32_t)(b.offsets[i + 1] - b.offsets[i]); if (U > w.max_len) w.max_len = U; }
    PairedBatch pb(o, ctx_for(o, fc, w.max_len), w);
    if (o.paths.paired_one_call && pb.np > 0 && pb.one_call()) return;
    pb.align_calls(); pb.emit_list();
    const std::vector<snapgpu_paired_result> &pu_res = pb.pu_res;
    const size_t nu = pu_res.size(), nrec = 2 * nu;
    size_pair_fields(o, w, nu, pb.su_res.size());
    if (nu == pb.np && pb.su_res.empty()) {                                 // one result per pair: one call over the batch as it is
        std::vector<int32_t> stale(nrec);
        with_growing_stride(w.rec, nrec, [&] {
            int rc = snapgpu_sam_fields_paired(pb.ctx, (uint32_t)nu, b.bases.data(), b.quals.data(), b.offsets.data(), pb.front_clip.data(), pb.data_len.data(), pu_res.data(),
                                               o.use_m ? 1 : 0, w.rec.flag.data(), w.rec.contig.data(), w.rec.pos.data(), w.rec.mapq.data(), w.rec.ops.data(), w.rec.ops_stride, w.rec.n_ops.data(),
                                               w.rec.nm.data(), w.rnext.data(), w.pnext.data(), w.tlen.data(), w.first_written.data(), stale.data());
            if (rc != SNAPGPU_OK) fail_rc(pb.ctx, "snapgpu_sam_fields_paired", rc);
        });
        return;
    }
    pb.rounds();
}

// ---------------------------------------------------------------------------------------- BAM (SNAPLib/Bam.cpp)
// One record as BAMFormat::writeRead / writePairs lay it out (Bam.cpp:1312-1508, 1033-1309): the same computed fields as the SAM line, binary.
//   refID / next_refID are ORIGINAL contig numbers (the header lists the contigs in the FASTA's order, Bam.cpp:1003-1021),
//   bin = reg2bin over the reference span of the cigar (an unmapped read: its mate's position, else -1; Bam.cpp:1473-1477),
//   aux: the default read group's fields (RG PL PU LB SM, Z), PG:Z:SNAP, NM:C (one byte: -1 reads as 255), and QS:i for mates (Bam.cpp:1510-1650).
static int bam_reg2bin(int beg, int end)                                   // Bam.cpp:523-535
{
    --end;
    if (beg >> 14 == end >> 14) return ((1 << 15) - 1) / 7 + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1 << 12) - 1) / 7 + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1 << 9) - 1) / 7 + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1 << 6) - 1) / 7 + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1 << 3) - 1) / 7 + (beg >> 26);
    return 0;
}
static inline void put_le32(std::string &o, uint32_t v) { char c[4] = {(char)(v & 0xff), (char)((v >> 8) & 0xff), (char)((v >> 16) & 0xff), (char)(v >> 24)}; o.append(c, 4); }
static const char BAM_RG_AUX[] = "RGZFASTQ\0PLZIllumina\0PUZpu\0LBZlb\0SMZsm";            // (+ the terminating NUL of the literal)
struct BamSeqCode { uint8_t c[256]; BamSeqCode() { memset(c, 0xf, 256); const char *t = "=ACMGRSVTWYHKDBN"; for (int i = 1; i < 16; i++) c[(unsigned char)t[i]] = (uint8_t)i; } };
static const BamSeqCode BAM_SEQ;                                             // Bam.cpp:505-510: anything unknown is N

static void put_bam_record(std::string &o, const std::vector<Contig> &contigs, const char *qname, size_t qn, int flag, int contig, long long pos1,
                           int mapq, const uint32_t *ops, int n_ops, int mate_contig, long long pnext1, long long tlen,
                           const char *s, const char *q, size_t U, int nm, bool with_qs, int qs)
{
    if (qn > 254) die("BAM format: QNAME must be shorter than 255 characters");
    const bool rc = (flag & 0x10) != 0;
    const int n_cig = n_ops > 0 ? n_ops : 0;
    static const int ref_base[16] = {1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};       // Bam.cpp:270
    int ref_len = n_cig > 0 ? 0 : (int)U;
    for (int c = 0; c < n_cig; c++) ref_len += ref_base[ops[c] & 0xf] * (int)(ops[c] >> 4);
    int bin;
    if (!(flag & 0x4)) bin = bam_reg2bin((int)pos1 - 1, (int)pos1 - 1 + ref_len);
    else if (with_qs && !(flag & 0x8)) bin = bam_reg2bin((int)pnext1 - 1, (int)pnext1);
    else bin = bam_reg2bin(-1, 0);
    const size_t aux_len = sizeof(BAM_RG_AUX) + 8 + 4 + (with_qs ? 7 : 0);
    const size_t block = 32 + (qn + 1) + 4 * (size_t)n_cig + (U + 1) / 2 + U + aux_len;     // without the block_size word itself
    const size_t at = o.size();
    o.reserve(at + 4 + block);
    put_le32(o, (uint32_t)block);
    put_le32(o, (uint32_t)(contig >= 0 ? contigs[(size_t)contig].orig : -1));
    put_le32(o, (uint32_t)((int)pos1 - 1));
    put_le32(o, ((uint32_t)bin << 16) | ((uint32_t)(mapq & 0xff) << 8) | (uint32_t)(qn + 1));
    put_le32(o, ((uint32_t)flag << 16) | (uint32_t)n_cig);
    put_le32(o, (uint32_t)U);
    put_le32(o, (uint32_t)(mate_contig >= 0 ? contigs[(size_t)mate_contig].orig : -1));
    put_le32(o, (uint32_t)((int)pnext1 - 1));
    put_le32(o, (uint32_t)(int)(tlen >= 0 ? (tlen & 0x7fffffff) : -((-tlen) & 0x7fffffff)));
    o.append(qname, qn); o.push_back('\0');
    for (int c = 0; c < n_cig; c++) put_le32(o, ops[c]);
    {   // SEQ (4 bits per base) and QUAL (Phred), in the record's orientation
        const size_t a0 = o.size();
        o.resize(a0 + (U + 1) / 2 + U);
        uint8_t *sq = (uint8_t *)&o[a0], *ql = sq + (U + 1) / 2;
        for (size_t j = 0; j < U; j++) {
            const char base = rc ? complement(s[U - 1 - j]) : s[j];
            const uint8_t code = BAM_SEQ.c[(unsigned char)base];
            if (j & 1) sq[j >> 1] |= code; else sq[j >> 1] = (uint8_t)(code << 4);
            ql[j] = (uint8_t)((rc ? q[U - 1 - j] : q[j]) - '!');
        }
    }
    o.append(BAM_RG_AUX, sizeof(BAM_RG_AUX));
    o.append("PGZSNAP", 8);
    o.append("NMC", 3); o.push_back((char)(uint8_t)nm);
    if (with_qs) { o.append("QSi", 3); put_le32(o, (uint32_t)qs); }
    if (o.size() - at != 4 + block) die("internal error: BAM record size");
}

// BGZF (SAM/BAM specification, section 4.1): gzip members of at most 64 KiB with the block size in an extra field; concatenated members
// are a valid gzip file, which is what lets every formatter thread compress its own batch.
static void bgzf_append(std::string &out, const char *data, size_t n)
{
    const size_t CHUNK = 0xff00;
    for (size_t at = 0; at < n || (n == 0 && at == 0); at += CHUNK) {
        const size_t len = n - at < CHUNK ? n - at : CHUNK;
        z_stream zs; memset(&zs, 0, sizeof(zs));
        if (deflateInit2(&zs, 1, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) die("deflateInit2 failed");
        std::vector<unsigned char> buf(len + len / 8 + 64);
        zs.next_in = (Bytef *)(data + at); zs.avail_in = (uInt)len; zs.next_out = buf.data(); zs.avail_out = (uInt)buf.size();
        if (deflate(&zs, Z_FINISH) != Z_STREAM_END) die("deflate failed");
        const size_t clen = buf.size() - zs.avail_out;
        deflateEnd(&zs);
        const size_t bsize = 18 + clen + 8;
        if (bsize > 0x10000) die("internal error: BGZF block too large");
        const unsigned char hdr[18] = {31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 'B', 'C', 2, 0, (unsigned char)((bsize - 1) & 0xff), (unsigned char)((bsize - 1) >> 8)};
        out.append((const char *)hdr, 18);
        out.append((const char *)buf.data(), clen);
        put_le32(out, (uint32_t)crc32(crc32(0L, Z_NULL, 0), (const Bytef *)(data + at), (uInt)len));
        put_le32(out, (uint32_t)len);
        if (n == 0) break;
    }
}

// ---------------------------------------------------------------------------------------- formatting stage
static inline void put_cigar(std::string &o, const Records &r, size_t i)
{
    if (r.n_ops[i] < 0) { o.push_back('*'); return; }
    const uint32_t *ops = r.cigar(i);
    for (int c = 0; c < r.n_ops[i]; c++) { put_uint(o, ops[c] >> 4); o.push_back("MIDNSHP=X"[ops[c] & 15]); }
}
static inline void put_seq_qual(std::string &o, const char *s, const char *q, size_t U, bool rc)
{
    const size_t at = o.size();
    o.resize(at + 2 * U + 1);
    char *d = &o[at];
    if (rc) { for (size_t j = 0; j < U; j++) { d[U - 1 - j] = complement(s[j]); d[U + 1 + U - 1 - j] = q[j]; } }
    else { memcpy(d, s, U); memcpy(d + U + 1, q, U); }
    d[U] = '\t';
}
static const char AUX_TAIL[] = "\tRG:Z:FASTQ\tPL:Z:Illumina\tPU:Z:pu\tLB:Z:lb\tSM:Z:sm";
struct ReadText { const char *s, *q; size_t U; const char *name; size_t name_len; };      // a read of the batch as it was parsed
static inline ReadText read_text(const Batch &b, size_t rd)
{
    return ReadText{b.bases.data() + b.offsets[rd], b.quals.data() + b.offsets[rd], (size_t)(b.offsets[rd + 1] - b.offsets[rd]), b.names.data() + b.name_off[rd], (size_t)(b.name_off[rd + 1] - b.name_off[rd])};
}
struct MateFields { int rnext; long long pnext, tlen; int qs; };          // what a mate's record has beyond a single-end one (rnext: -1 "*", -2 "=", else a contig)
// record i of `r` for read `rd`, as a SAM line or a BAM record; QNAME: the first qn bytes of the read's name, cut at a space ("illegal in
// SAM: truncate at the space", SAM.cpp:2001-2004); m: the mate fields and QS of a pair's record, NULL for a record without a mate
static inline void put_record(std::string &o, const std::vector<Contig> &contigs, bool bam, const Records &r, size_t i, const ReadText &rd, size_t qn, const MateFields *m)
{
    const void *sp = memchr(rd.name, ' ', qn);
    if (sp) qn = (size_t)((const char *)sp - rd.name);
    if (bam) {
        put_bam_record(o, contigs, rd.name, qn, r.flag[i], r.contig[i], r.pos[i], r.mapq[i], r.cigar(i), r.n_ops[i], m ? (m->rnext == -2 ? r.contig[i] : m->rnext) : -1,
                       m ? m->pnext : 0, m ? m->tlen : 0, rd.s, rd.q, rd.U, r.nm[i], m != NULL, m ? m->qs : 0);
        return;
    }
    o.append(rd.name, qn); o.push_back('\t'); put_int(o, r.flag[i]); o.push_back('\t');
    if (r.contig[i] >= 0) o += contigs[(size_t)r.contig[i]].name; else o.push_back('*');
    o.push_back('\t'); put_int(o, r.pos[i]); o.push_back('\t'); put_int(o, r.mapq[i]); o.push_back('\t');
    put_cigar(o, r, i);
    if (m) {
        o.push_back('\t');
        if (m->rnext == -2) o.push_back('='); else if (m->rnext >= 0) o += contigs[(size_t)m->rnext].name; else o.push_back('*');
        o.push_back('\t'); put_int(o, m->pnext); o.push_back('\t'); put_int(o, (int)m->tlen); o.push_back('\t');
    } else o += "\t*\t0\t0\t";
    put_seq_qual(o, rd.s, rd.q, rd.U, (r.flag[i] & 0x10) != 0);
    o += "\tPG:Z:SNAP\tNM:i:"; put_int(o, r.nm[i]); o += AUX_TAIL;
    if (m) { o += "\tQS:i:"; put_int(o, m->qs); }
    o.push_back('\n');
}

static void format_single(const std::vector<Contig> &contigs, Work &w)
{
    std::string &o = w.text;
    o.clear(); o.reserve(w.rec_read.size() * 420);
    for (size_t i = 0; i < w.rec_read.size(); i++) {
        const ReadText rd = read_text(w.b, w.rec_read[i]);
        put_record(o, contigs, w.bam, w.rec, i, rd, rd.name_len, NULL);
        w.mapped += (w.rec.flag[i] & 0x4) == 0;
    }
}

static void format_paired(const std::vector<Contig> &contigs, Work &w)
{
    const Batch &b = w.b;
    std::string &o = w.text;
    o.clear(); o.reserve(w.emit.size() * 880);
    for (const Work::Emit &e : w.emit) {
        if (e.single) {
            // a mate's single-end secondary result: SAMFormat::writeRead without a mate -- the whole read id (the "/1" stays: the call is given
            // getIdLength(), ReadWriter.cpp:521), no mate fields, no QS
            const ReadText rd = read_text(b, w.su_read[e.unit]);
            put_record(o, contigs, w.bam, w.srec, e.unit, rd, rd.name_len, NULL);
            w.mapped += (w.srec.flag[e.unit] & 0x4) == 0;
            continue;
        }
        const size_t u = e.unit, k = w.pu_pair[u];
        // QNAME: the /1 /2 suffixes go when both names carry them (ReadWriter.cpp:392-404)
        const char *n0 = b.names.data() + b.name_off[2 * k], *n1 = b.names.data() + b.name_off[2 * k + 1];
        size_t idl[2] = { (size_t)(b.name_off[2 * k + 1] - b.name_off[2 * k]), (size_t)(b.name_off[2 * k + 2] - b.name_off[2 * k + 1]) };
        if (idl[0] == idl[1] && idl[0] > 2 && n0[idl[0] - 2] == '/' && n1[idl[0] - 2] == '/') {
            const char c0 = n0[idl[0] - 1], c1 = n1[idl[1] - 1];
            if ((c0 == '1' || c0 == '2') && (c1 == '1' || c1 == '2') && c0 != c1) { idl[0] -= 2; idl[1] -= 2; }
        }
        for (int ord = 0; ord < 2; ord++) {
            const int v = ord == 0 ? w.first_written[u] : 1 - w.first_written[u];
            const size_t i = 2 * u + (size_t)v;                                             // fields
            const ReadText rd = read_text(b, 2 * k + (size_t)v), mate = read_text(b, 2 * k + (size_t)(1 - v));
            int mqs = 0;                                                // QS: the mate's qualities >= 15, summed (SAM.cpp:1826-1837)
            for (size_t j = 0; j < mate.U; j++) { const int x = (int)(unsigned char)mate.q[j] - '!'; mqs += x >= 15 ? (x != 255) * x : 0; }
            const MateFields m = {w.rnext[i], w.pnext[i], w.tlen[i], mqs};
            put_record(o, contigs, w.bam, w.rec, i, rd, idl[v], &m);
            w.mapped += (w.rec.flag[i] & 0x4) == 0;
        }
    }
}

// ---------------------------------------------------------------------------------------- main
// ---------------------------------------------------------------------------------------- -so: sorted runs and their merge
// Every batch becomes one run: its BAM records in key order (snap_amd/csrc/bam_sort.h: key = (uint32) refID << 32 | (uint32)(pos + 1), ties in
// input order) and their keys.  Runs are kept in batch order; a run that would take the bytes held in memory past -sm goes uncompressed to
// <out>.sort.tmp (its keys, 8 bytes a record, stay) and is read back in pieces.  The merge takes the smallest (key, run number), so a tie goes to
// the lower batch: the file is the stable sort of the input-order record stream whatever -gpus, -q, -t or -b are.
static inline uint32_t get_le32(const char *p) { return (uint32_t)(unsigned char)p[0] | ((uint32_t)(unsigned char)p[1] << 8) | ((uint32_t)(unsigned char)p[2] << 16) | ((uint32_t)(unsigned char)p[3] << 24); }
// a batch that did not come down sorted: its records through snapgpu_bam_sort on the context the formatter threads share
static void sort_run(snapgpu_ctx *ctx, std::mutex &m, Work &w)
{
    std::vector<uint64_t> bb(1, 0);
    for (size_t at = 0; at < w.text.size();) {
        if (w.text.size() - at < 4) die("internal error: a BAM record is cut short");
        at += 4 + (size_t)get_le32(w.text.data() + at);
        if (at > w.text.size()) die("internal error: a BAM record is cut short");
        bb.push_back(at);
    }
    const size_t n = bb.size() - 1;
    std::string sorted(w.text.size(), '\0');
    std::vector<uint64_t> sb(n + 1);
    w.keys.assign(n, 0);
    if (n) {
        std::lock_guard<std::mutex> l(m);
        const int rc = snapgpu_bam_sort(ctx, n, (const uint8_t *)w.text.data(), bb.data(), (uint8_t *)&sorted[0], sb.data(), w.keys.data(), NULL);
        if (rc != SNAPGPU_OK) fail_rc(ctx, "snapgpu_bam_sort", rc);
    }
    w.text.swap(sorted); w.sort_done = true;
}
struct SortRun {
    std::string bytes; std::vector<uint64_t> keys; uint64_t n_bytes = 0, file_at = 0; bool spilled = false;
    // the merge's cursor
    size_t next = 0; uint64_t at = 0; std::vector<char> piece; uint64_t piece_at = 0;
};
struct SortRuns {
    std::vector<SortRun> runs; uint64_t held = 0, limit = 0, tmp_bytes = 0, n_spilled = 0, n_records = 0;
    std::string tmp_path; FILE *tmp = NULL;
    void add(Work &w) {
        runs.emplace_back();
        SortRun &r = runs.back();
        size_t n = 0;
        for (size_t at = 0; at < w.text.size(); n++) at += 4 + (size_t)get_le32(w.text.data() + at);
        if (w.keys.size() < n) die("internal error: a sorted run has fewer keys than records");
        r.keys.assign(w.keys.begin(), w.keys.begin() + (ptrdiff_t)n); r.n_bytes = w.text.size(); n_records += n;
        if (held + r.n_bytes > limit) {
            if (!tmp) { if (!(tmp = fopen(tmp_path.c_str(), "w+b"))) die("cannot create ", tmp_path.c_str()); g_sort_tmp_path = tmp_path; }
            if (fseeko(tmp, (off_t)tmp_bytes, SEEK_SET) != 0 || fwrite(w.text.data(), 1, w.text.size(), tmp) != w.text.size()) die("write error on ", tmp_path.c_str());
            r.spilled = true; r.file_at = tmp_bytes; tmp_bytes += r.n_bytes; n_spilled++;
        } else { r.bytes.swap(w.text); held += r.n_bytes; }                      // (the batch goes back to the pool next: its buffer stays with the run)
    }
    // the next record of run r: where it is and how long
    const char *record(SortRun &r, size_t &len) {
        if (!r.spilled) { len = 4 + (size_t)get_le32(r.bytes.data() + r.at); return r.bytes.data() + r.at; }
        auto have = [&](uint64_t need) { return r.at >= r.piece_at && r.at + need <= r.piece_at + r.piece.size(); };
        auto fill = [&](uint64_t need) {
            const uint64_t PIECE = 1u << 20, left = r.n_bytes - r.at, want = need > PIECE ? need : PIECE;
            r.piece.resize((size_t)(want < left ? want : left)); r.piece_at = r.at;
            if (fseeko(tmp, (off_t)(r.file_at + r.at), SEEK_SET) != 0 || fread(r.piece.data(), 1, r.piece.size(), tmp) != r.piece.size()) die("read error on ", tmp_path.c_str());
        };
        if (!have(4)) fill(4);
        len = 4 + (size_t)get_le32(r.piece.data() + (r.at - r.piece_at));
        if (!have(len)) fill(len);
        return r.piece.data() + (r.at - r.piece_at);
    }
    // the k-way merge; emit(data, n) takes the merged stream in pieces that are multiples of 0xff00 bytes but for the last
    template <class Emit> void merge(Emit emit) {
        if (tmp) fflush(tmp);
        typedef std::pair<uint64_t, size_t> Head;                        // (key, run): the smaller run number wins a tie
        std::priority_queue<Head, std::vector<Head>, std::greater<Head>> heap;
        for (size_t i = 0; i < runs.size(); i++) if (!runs[i].keys.empty()) heap.push(Head(runs[i].keys[0], i));
        const size_t FLUSH = 64 * (size_t)0xff00;
        std::string buf; buf.reserve(FLUSH + (1u << 16));
        while (!heap.empty()) {
            const size_t i = heap.top().second; heap.pop();
            SortRun &r = runs[i];
            size_t len = 0;
            const char *p = record(r, len);
            buf.append(p, len);
            r.at += len; r.next++;
            if (r.next < r.keys.size()) heap.push(Head(r.keys[r.next], i));
            else { std::string().swap(r.bytes); std::vector<char>().swap(r.piece); }
            if (buf.size() >= FLUSH) { const size_t k = buf.size() / 0xff00 * 0xff00; emit(buf.data(), k); buf.erase(0, k); }
        }
        if (!buf.empty()) emit(buf.data(), buf.size());
    }
    void finish() { if (tmp) { fclose(tmp); tmp = NULL; (void)unlink(tmp_path.c_str()); g_sort_tmp_path.clear(); } }
};

int main(int argc, char **argv)
{
    Options o;
    o.paired = argc >= 2 && strcmp(argv[1], "paired") == 0;
    if (argc < (o.paired ? 5 : 4) || (!o.paired && strcmp(argv[1], "single") != 0))
        die("usage: snapgpu-sam single <index-dir> <reads.fq> -o <out.sam|out.bam> | paired <index-dir> <r1.fq> <r2.fq> -o <out.sam|out.bam>  [-d N] [-G-] [-=] [-M] [-om N] [-omax N] [-mpc N] [-ae] [-ea] [-mrl N] [-b N] [-gpus N] [-q N] [-t N] [-so [-sm GB]]");
    const std::string index_dir = argv[2], fastq = argv[3], fastq2 = o.paired ? argv[4] : "";
    std::string out_path;
    snapgpu_default_params(&o.p);
    o.p.max_read_len = 400;                                                // per-wave buffers; SNAPGPU_MAX_READ_LEN raises it (<= 1000), as for snap-aligner-gpu
    if (const char *e = getenv("SNAPGPU_MAX_READ_LEN")) { const int v = atoi(e); if (v >= 50 && v <= 1000) o.p.max_read_len = (uint32_t)v; }
    std::string cl = argv[1];
    for (int i = 2; i < argc; i++) { cl += " "; cl += argv[i]; }
    for (int i = o.paired ? 5 : 4; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-o" && i + 1 < argc) out_path = argv[++i];
        else if (a == "-d" && i + 1 < argc) o.p.max_k = (uint32_t)atoi(argv[++i]);
        else if (a == "-G-") o.p.use_affine_gap = 0;
        else if (a == "-=") o.use_m = false;
        else if (a == "-M") o.use_m = true;
        else if (a.size() == 4 && a.compare(0, 2, "-C") == 0 && strchr("+-", a[2]) && strchr("+-", a[3])) { o.clip_front = a[2] == '+'; o.clip_back = a[3] == '+'; }   // AlignerOptions.cpp: -Cxx
        else if (a == "-om" && i + 1 < argc) o.om = atoi(argv[++i]);                       // secondary alignments (AlignerOptions.cpp:70-72)
        else if (a == "-omax" && i + 1 < argc) o.omax = atoll(argv[++i]);
        else if (a == "-mpc" && i + 1 < argc) o.mpc = atoi(argv[++i]);
        else if (a == "-ae") o.ae = true;                                                    // AlignerOptions.cpp:476
        else if (a == "-f") o.stop_on_first_hit = true;                                      // AlignerOptions.cpp:573
        else if (a == "-x") o.explore_popular_seeds = true;                                  // AlignerOptions.cpp:570
        else if (a == "-ea") o.p.emit_alt_alignments = 1;                                  // the first ALT alignment as an extra record (SingleAligner.cpp:320-322)
        else if (a == "-D" && i + 1 < argc) o.p.extra_search_depth = (uint32_t)atoi(argv[++i]);
        else if (a == "-mrl" && i + 1 < argc) o.min_read_len = (unsigned)atoi(argv[++i]);
        else if (a == "-b" && i + 1 < argc) o.batch_reads = (size_t)atoll(argv[++i]);
        else if (a == "-g" && i + 1 < argc) o.group = (size_t)atoll(argv[++i]);
        else if (a == "-gpus" && i + 1 < argc) o.n_gpus = atoi(argv[++i]);
        else if (a == "-q" && i + 1 < argc) o.ctx_per_gpu = atoi(argv[++i]);
        else if (a == "-t" && i + 1 < argc) o.n_format = atoi(argv[++i]);  // host threads that format records (the reference's -t counts aligner threads)
        else if (a == "-tp" && i + 1 < argc) o.n_parse = atoi(argv[++i]);  // host threads that parse a plain FASTQ file
        else if (a == "-so") o.sorted = true;                                                // AlignerOptions.cpp: sort the output by coordinate
        else if (a == "-sm" && i + 1 < argc) o.sort_gb = atof(argv[++i]);                  // GB of sorted runs held in memory (the reference's -sm sizes its sort buffers)
        else if (a == "-seqread") o.seqread = true;
        else if (a == "-passes" && i + 1 < argc) o.passes = atoi(argv[++i]);   // (measurement: the whole FASTQ -> SAM stream N times over the resident index; the output is the last pass's)
        else die("option not supported: ", a.c_str());
    }
    if (out_path.empty()) die("-o <out.sam | out.bam> is required");
    if (o.ae && o.paired) die("-ae is implemented for `single` only (the paired-end aligners' use of AlignmentAdjuster is not: DESIGN.md section 16)");
    if (o.ae && o.clip_front) die("-ae with front clipping (-C+x) is not supported: the adjuster is restated for reads the reader has not clipped at the front");
    o.bam = out_path.size() > 4 && out_path.compare(out_path.size() - 4, 4, ".bam") == 0;     // by extension, like the reference (AlignerOptions.cpp)
    if (o.sorted && !o.bam) die("-so writes a coordinate-sorted BAM file: -o must end in .bam (sorted SAM text is not implemented)");
    if (o.sorted && !(o.sort_gb >= 0 && o.sort_gb <= 1048576.0)) die("-sm must be between 0 and 1048576 (GB)");
    choose_paths(o);
    const bool batch_auto = o.batch_reads == 0;
    if (batch_auto) o.batch_reads = 262144;                                // (the mapped reader, which knows the file's size, picks below)
    if (o.batch_reads < (o.paired ? 2u : 1u)) die("-b must be at least 1 (2 for paired)");
    if (o.paired) o.batch_reads &= ~(size_t)1;
    // feeders per GPU: a launch lasts as long as its slowest read (~150 ms when the batch holds one of the heavy ones), so batches of 131 072
    // reads need several launches in flight to keep the chip busy: 20 M reads go through at 2.24 / 2.47 / 2.50 M reads/s with 3 / 6 / 8
    // feeders (profiles/r04zy).  The paired-end launches are long already.
    // Round 5: the GPU gets ~1 M single-end reads per call (gpu_single_group: bench.py's launch size -- the tail of a launch then costs 10 %,
    // not half of it) through ONE call (snapgpu_align_sam_single) and the 192-position kernel variant: three feeders cover the
    // copies of one batch with the kernels of the others (20 M reads: 4.78 / 4.56 / 4.74 M reads/s with 3 / 4 / 6 feeders, profiles/r05g).
    if (o.ctx_per_gpu == 0) o.ctx_per_gpu = 3;
    if (o.ctx_per_gpu < 1 || o.ctx_per_gpu > 8) die("-q must be in [1, 8]");
    // cigar ops per record: about 2 * edits + soft clips; grown on demand when a record needs more (with_growing_stride)
    { uint32_t need = 2 * (o.p.max_k + o.p.extra_search_depth) + 8; o.ops_stride = (need + 3u) & ~3u; if (o.ops_stride < 16) o.ops_stride = 16; }

    const auto t_process = std::chrono::steady_clock::now();
    std::vector<Contig> contigs; uint64_t n_bases = 0; uint32_t padding = 0;
    load_contigs(index_dir, contigs, n_bases, padding);
    g_contigs = &contigs; g_n_bases = n_bases; g_padding = padding;

    // ---- contexts: GPU 0 reads the index, the other GPUs get it over RCCL, every further feeder on a GPU shares that GPU's blobs
    int visible = snapgpu_device_count();
    if (visible <= 0) { snapgpu_ctx *none = NULL; int rc = snapgpu_create_from_directory(index_dir.c_str(), &o.p, 0, &none); fail_rc(none, "snapgpu_create_from_directory", rc); }
    if (o.n_gpus <= 0 || o.n_gpus > visible) o.n_gpus = visible;
    std::vector<snapgpu_ctx *> primary((size_t)o.n_gpus, NULL);
    snapgpu_default_paired_params(&o.pp);
    o.pp.min_read_length = o.min_read_len;
    for (const Contig &c : contigs) if (c.is_alt) g_index_has_alt = true;
    // every context starts in read-length class 0 (FeederCtx): the index owner too
    snapgpu_params p0 = o.p; p0.max_read_len = class_len(o, 0);
    int rc = snapgpu_create_from_directory(index_dir.c_str(), &p0, 0, &primary[0]);
    if (rc != SNAPGPU_OK) fail_rc(primary[0], "snapgpu_create_from_directory", rc);
    for (int g = 1; g < o.n_gpus; g++) {
        rc = snapgpu_create_replica(primary[0], g, 0, &primary[(size_t)g]);
        if (rc != SNAPGPU_OK) fail_rc(primary[0], "snapgpu_create_replica", rc);
    }
    if (o.n_gpus > 1) {
        rc = snapgpu_broadcast_index(primary.data(), o.n_gpus);
        if (rc != SNAPGPU_OK) fail_rc(primary[0], "snapgpu_broadcast_index", rc);
    }
    // -so: the formatter threads' snapgpu_bam_sort calls and the merge's snapgpu_bgzf_compress run on GPU 0's first context, which its first feeder
    // uses too: calls on a context are serial, so that feeder holds sort_m while it works (a context of their own does not fit beside the
    // feeders' secondary-result pools of a paired -om run)
    snapgpu_ctx *sort_ctx = o.sorted ? primary[0] : NULL; std::mutex sort_m;
    std::vector<FeederCtx> fctx;                                            // one per feeder thread
    for (int g = 0; g < o.n_gpus; g++) {
        for (int k = 0; k < o.ctx_per_gpu; k++) {
            FeederCtx f; f.owner = primary[(size_t)g]; f.device = g;
            if (k == 0) f.c[0] = primary[(size_t)g];
            else {
                rc = snapgpu_create_replica(primary[(size_t)g], g, 1, &f.c[0]);
                if (rc != SNAPGPU_OK) fail_rc(primary[(size_t)g], "snapgpu_create_replica", rc);
            }
            configure_ctx(o, f.c[0]);
            fctx.push_back(f);
        }
    }
    const bool merge_on_device = o.sorted && env_switch("SNAPGPU_SAM_DEVICE_BGZF", false);
    unsigned long long sort_runs = 0, sort_records = 0, sort_spilled = 0; double s_merge = 0.0;
    // host threads: formatting a record is ~1 us of text work, so one GPU's ~5 M records/s want a few dozen formatters (the cap of 16 of
    // rounds 2-3 was the pipeline's bottleneck on a 256-thread host); parsers likewise
    { const unsigned hc = std::thread::hardware_concurrency() ? std::thread::hardware_concurrency() : 8;
      if (o.n_format <= 0) { unsigned v = hc / 3; o.n_format = (int)(v < 4 ? 4 : (v > 64 ? 64 : v)); }
      if (o.n_parse <= 0) { unsigned v = hc / 8; o.n_parse = (int)(v < 2 ? 2 : (v > 24 ? 24 : v)); } }

    if (o.passes < 1 || o.passes > 100) die("-passes must be in [1, 100]");
    unsigned long long total = 0, mapped = 0;
    bool use_map = false;
    auto t_ready = std::chrono::steady_clock::now();
    double s_load = 0.0;
    std::vector<double> pass_s;
    WorkPool pool(256);
    for (int pass = 0; pass < o.passes; pass++) {
        g_bam_batches = 0; g_bam_records = 0; g_bgzf_batches = 0; g_bgzf_members = 0; g_bgzf_in = 0; g_bgzf_out = 0;
    total = 0; mapped = 0;
    if (pass > 0) (void)unlink(out_path.c_str());        // (-passes: the previous pass's output goes BEFORE this pass is timed -- replacing a 5.6 GB file at the end of a pass
                                                         //  cost it 1.3 s of page-cache work that streaming a FASTQ file into a new SAM file does not have: profiles/r06j)
    const std::string partial_path = out_path + ".partial";
    FILE *out = fopen(partial_path.c_str(), "wb");
    if (!out) die("cannot create ", partial_path.c_str());
    g_partial_path = partial_path;
    setvbuf(out, NULL, _IOFBF, 8u << 20);
    // header (SAM.cpp:1232-1295); @SQ lines go by ORIGINAL contig number: the index builder moves ALT contigs behind the regular ones
    // (FASTA.cpp:359-384), the header keeps the FASTA's order (getContigByOriginalContigNumber, SAM.cpp:1291)
    // The BAM header is the same text inside the binary header, followed by the contig table in the same (original) order (Bam.cpp:970-1031).
    {
        std::string text = std::string("@HD\tVN:1.6\t") + (o.sorted ? "SO:coordinate" : "GO:query") + "\n@RG\tID:FASTQ\tPL:Illumina\tPU:pu\tLB:lb\tSM:sm\n@PG\tID:SNAP\tPN:SNAP\tCL:" + cl + "\tVN:2.0.5\n";
        std::string refs;
        std::vector<size_t> by_orig(contigs.size());
        bool perm = true;
        std::vector<char> seen(contigs.size(), 0);
        for (size_t c = 0; c < contigs.size(); c++) { if (contigs[c].orig < 0 || (size_t)contigs[c].orig >= contigs.size() || seen[(size_t)contigs[c].orig]) { perm = false; break; } seen[(size_t)contigs[c].orig] = 1; by_orig[(size_t)contigs[c].orig] = c; }
        if (o.bam && !perm) die("the index's original contig numbers are not a permutation: cannot number the BAM reference sequences");
        for (size_t k = 0; k < contigs.size(); k++) {
            const size_t c = perm ? by_orig[k] : k;
            const uint64_t end = c + 1 < contigs.size() ? contigs[c + 1].begin : n_bases;
            const unsigned long long len = (unsigned long long)(end - contigs[c].begin - padding);
            text += "@SQ\tSN:" + contigs[c].name + "\tLN:" + std::to_string(len) + (contigs[c].is_alt ? "\tAH:*" : "") + "\n";
            put_le32(refs, (uint32_t)contigs[c].name.size() + 1); refs += contigs[c].name; refs.push_back('\0'); put_le32(refs, (uint32_t)len);
        }
        if (o.bam) {
            std::string h = "BAM\1";
            put_le32(h, (uint32_t)text.size()); h += text; put_le32(h, (uint32_t)contigs.size()); h += refs;
            std::string z; bgzf_append(z, h.data(), h.size());
            if (fwrite(z.data(), 1, z.size(), out) != z.size()) die("write error on ", out_path.c_str());
        } else if (fwrite(text.data(), 1, text.size(), out) != text.size()) die("write error on ", out_path.c_str());
    }

    t_ready = std::chrono::steady_clock::now();                             // the index is resident, the contexts exist: the streaming part starts here
    if (pass == 0) s_load = std::chrono::duration<double>(t_ready - t_process).count();
    // ---- the pipeline
    // single-end batches per GPU call: enough to make ~1 M reads, but never so many that the feeders of a small file have nothing to share
    size_t group = o.group ? o.group : (o.paired ? 1 : 8);
    if (group < 1) group = 1;
    if (group > 64) group = 64;
    Queue<Work *> q_parsed(fctx.size() * (o.paired ? 2 : group + 2) + 2), q_aligned((size_t)o.n_format * 2 + 2 + group * fctx.size());
    std::mutex done_m; std::condition_variable done_cv; std::map<uint64_t, Work *> done;
    std::atomic<uint64_t> n_batches(0); std::atomic<bool> reader_done(false);

    // ---- input: a plain FASTQ file is mapped, indexed by line count and parsed batch by batch by o.n_parse threads; gzip input, -seqread
    // and files whose lines do not come in fours go through the sequential reader
    MappedFastq mf, mf2;
    use_map = !o.seqread && mf.open(fastq.c_str()) && (!o.paired || mf2.open(fastq2.c_str()));
    if (use_map) {
        const auto t0 = std::chrono::steady_clock::now();
        use_map = mf.index(o.n_parse) && (!o.paired || mf2.index(o.n_parse));
        if (use_map && o.paired && mf.n_lines != mf2.n_lines) die(mf.n_lines > mf2.n_lines ? "the second FASTQ file has fewer reads than the first" : "the second FASTQ file has more reads than the first");
        if (use_map && o.verbose) fprintf(stderr, "snapgpu-sam: %llu FASTQ records indexed in %.2f s\n", (unsigned long long)(mf.n_lines / 4), std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    if (!use_map) { mf.close(); mf2.close(); }
    std::vector<std::thread> parsers;
    std::thread reader;
    if (use_map) {
        const uint64_t n_records = mf.n_lines / 4;
        if (batch_auto && o.paired) {       // enough batches to keep every feeder busy (four each), each as large as that allows: 64 K .. 512 K reads
            uint64_t v = 2 * n_records / (4 * (uint64_t)fctx.size());
            v = v < 65536 ? 65536 : (v > 524288 ? 524288 : v);
            o.batch_reads = (size_t)(v & ~(uint64_t)1);
        } else if (batch_auto) o.batch_reads = 131072;       // (single end: small batches for the host stages, grouped for the GPU: gpu_single_group)
        const uint64_t per_batch = o.paired ? o.batch_reads / 2 : o.batch_reads;           // records of EACH file per batch
        const uint64_t n_units = (n_records + per_batch - 1) / per_batch;
        n_batches = n_units; reader_done = true;
        // (a small file: no feeder takes more batches per call than leaves the others their share -- with every batch available at once the first feeder
        //  to wake would otherwise take eight and a file of a million reads would run on one feeder of one GPU)
        if (!o.group) { const size_t share = (size_t)(n_units / (uint64_t)fctx.size()); if (group > (share ? share : 1)) group = share ? share : 1; }
        std::shared_ptr<std::atomic<uint64_t>> next_unit = std::make_shared<std::atomic<uint64_t>>(0);
        std::shared_ptr<std::atomic<int>> parsers_left = std::make_shared<std::atomic<int>>(o.n_parse);
        for (int t = 0; t < o.n_parse; t++)
            parsers.emplace_back([&, next_unit, parsers_left, n_records, per_batch, n_units] {
                for (;;) {
                    const uint64_t u = next_unit->fetch_add(1);
                    if (u >= n_units) break;
                    const uint64_t r0 = u * per_batch, r1 = r0 + per_batch < n_records ? r0 + per_batch : n_records;
                    Work *w = pool.get();
                    StageTimer *pt = new StageTimer(g_ns_parse);
                    w->b.clear(); w->b.seq = u; w->bam = o.bam;
                    size_t at = mf.line_start(4 * r0), at2 = o.paired ? mf2.line_start(4 * r0) : 0;
                    for (uint64_t r = r0; r < r1; r++) {
                        at = parse_mapped_record(mf, at, w->b, o.p.max_read_len);
                        if (o.paired) at2 = parse_mapped_record(mf2, at2, w->b, o.p.max_read_len);
                    }
                    if (!o.paired) prepare_single(o, *w);
                    delete pt;
                    q_parsed.push(w);
                }
                if (--*parsers_left == 0) { q_parsed.close(); std::lock_guard<std::mutex> l(done_m); done_cv.notify_all(); }
            });
    } else
    reader = std::thread([&] {
        LineReader in, in2;
        in.open(fastq.c_str());
        if (o.paired) in2.open(fastq2.c_str());
        uint64_t seq = 0;
        bool eof = false;
        while (!eof) {
            Work *w = pool.get();
            w->b.clear(); w->b.seq = seq; w->bam = o.bam;
            while (w->b.n() < o.batch_reads) {
                if (!next_read(in, w->b, o.p.max_read_len)) { eof = true; break; }
                if (o.paired && !next_read(in2, w->b, o.p.max_read_len)) die("the second FASTQ file has fewer reads than the first");
            }
            if (eof && o.paired) { Batch probe; probe.clear(); if (next_read(in2, probe, o.p.max_read_len)) die("the second FASTQ file has more reads than the first"); }
            if (w->b.n() == 0) { pool.put(w); break; }
            seq++;
            q_parsed.push(w);
        }
        in.close(); in2.close();
        n_batches = seq; reader_done = true;
        q_parsed.close();
        { std::lock_guard<std::mutex> l(done_m); done_cv.notify_all(); }
    });
    std::vector<std::thread> feeders, formatters;
    std::atomic<int> feeders_left((int)fctx.size());
    for (size_t t = 0; t < fctx.size(); t++)
        feeders.emplace_back([&, t] {
            if (o.paired) {
                Work *w;
                while (q_parsed.pop(w)) {
                    { std::unique_lock<std::mutex> hold(sort_m, std::defer_lock); if (o.sorted && t == 0) hold.lock(); gpu_paired(o, fctx[t], *w); }
                    q_aligned.push(w);
                }
            } else {
                GroupBuf gb; std::vector<Work *> ws;
                for (;;) {
                    ws.clear();
                    { StageTimer st(g_ns_wait_in); if (q_parsed.pop_upto(ws, group, std::chrono::milliseconds(20)) == 0) break; }
                    { std::unique_lock<std::mutex> hold(sort_m, std::defer_lock); if (o.sorted && t == 0) hold.lock(); gpu_single_group(o, fctx[t], ws, gb); }
                    { StageTimer st(g_ns_wait_out); for (Work *w : ws) q_aligned.push(w); }
                }
            }
            if (--feeders_left == 0) q_aligned.close();
        });
    for (int t = 0; t < o.n_format; t++)
        formatters.emplace_back([&] {
            Work *w;
            while (q_aligned.pop(w)) {
                if (!w->text_done) { StageTimer st(g_ns_format); if (o.paired) format_paired(contigs, *w); else format_single(contigs, *w); }
                if (o.sorted) { if (!w->sort_done) sort_run(sort_ctx, sort_m, *w); }
                else if (o.bam && !w->bgzf_done) { std::string z; z.reserve(w->text.size() / 3 + 64); bgzf_append(z, w->text.data(), w->text.size()); w->text.swap(z); }
                std::lock_guard<std::mutex> l(done_m); done[w->b.seq] = w; done_cv.notify_all();
            }
        });
    SortRuns sr; sr.limit = (uint64_t)(o.sort_gb * 1073741824.0); sr.tmp_path = out_path + ".sort.tmp";
    const auto t_pipe = std::chrono::steady_clock::now();
    double t_first_s = -1.0;
    for (uint64_t next = 0;; next++) {                                      // the writer: batches in input order
        Work *w = NULL;
        {
            StageTimer st(g_ns_wait_writer);
            std::unique_lock<std::mutex> l(done_m);
            done_cv.wait(l, [&] { return done.count(next) || (reader_done && next >= n_batches); });
            if (!done.count(next)) break;
            w = done[next]; done.erase(next);
        }
        if (o.sorted) { StageTimer st(g_ns_write); sr.add(*w); }
        else { StageTimer st(g_ns_write); if (fwrite(w->text.data(), 1, w->text.size(), out) != w->text.size()) die("write error on ", out_path.c_str()); }
        if (t_first_s < 0) t_first_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_ready).count();
        total += w->b.n(); mapped += w->mapped;
        pool.put(w);
    }
    const auto t_written = std::chrono::steady_clock::now();
    if (reader.joinable()) reader.join();
    for (auto &t : parsers) t.join();
    mf.close(); mf2.close();
    for (auto &t : feeders) t.join();
    for (auto &t : formatters) t.join();
    const auto t_joined = std::chrono::steady_clock::now();
    if (o.sorted) {                                                          // the merged stream through BGZF: zlib, or the device's coder under SNAPGPU_SAM_DEVICE_BGZF=1
        std::string z; std::vector<uint64_t> member_begin;
        sr.merge([&](const char *data, size_t n) {
            z.clear();
            if (merge_on_device) {
                const uint64_t nm = (n + 0xff00 - 1) / 0xff00;
                z.resize((size_t)nm * (0xff00 + 31)); member_begin.resize((size_t)nm + 1);
                uint64_t n_members = 0, out_bytes = 0;
                const int zrc = snapgpu_bgzf_compress(sort_ctx, n, (const uint8_t *)data, 0xff00, z.size(), (uint8_t *)&z[0], member_begin.data(), &n_members, &out_bytes);
                if (zrc != SNAPGPU_OK) fail_rc(sort_ctx, "snapgpu_bgzf_compress", zrc);
                z.resize((size_t)out_bytes);
            } else bgzf_append(z, data, n);
            if (fwrite(z.data(), 1, z.size(), out) != z.size()) die("write error on ", out_path.c_str());
        });
        sr.finish();
        sort_runs = sr.runs.size(); sort_records = sr.n_records; sort_spilled = sr.n_spilled;
        s_merge = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_joined).count();
    }
    if (o.bam) { std::string eof; bgzf_append(eof, "", 0); if (fwrite(eof.data(), 1, eof.size(), out) != eof.size()) die("write error on ", out_path.c_str()); }     // the empty end-of-file block
    if (fclose(out) != 0) die("write error on ", out_path.c_str());
    if (rename(partial_path.c_str(), out_path.c_str()) != 0) die("cannot rename the finished output to ", out_path.c_str());
    g_partial_path.clear();
    pass_s.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t_ready).count());
    if (o.verbose)
        fprintf(stderr, "snapgpu-sam: pass %d timeline: pipeline up at %.3f s, first batch written at %.3f s, last at %.3f s, threads joined at %.3f s, file closed and renamed at %.3f s\n", pass + 1,
                std::chrono::duration<double>(t_pipe - t_ready).count(), t_first_s, std::chrono::duration<double>(t_written - t_ready).count(),
                std::chrono::duration<double>(t_joined - t_ready).count(), pass_s.back());
    if (o.passes > 1) fprintf(stderr, "snapgpu-sam: pass %d of %d: %llu reads in %.3f s = %.0f reads/s\n", pass + 1, o.passes, total, pass_s.back(), pass_s.back() > 0 ? (double)total / pass_s.back() : 0.0);
    }
    for (size_t t = fctx.size(); t-- > 0;) {                                // sharers before the owner of the blobs they share
        for (int k = 2; k >= 0; k--) {
            snapgpu_ctx *c = fctx[t].c[k];
            if (!c || c == fctx[t].owner) continue;
            bool seen = false; for (int j = 0; j < k; j++) seen = seen || fctx[t].c[j] == c;
            if (!seen) snapgpu_destroy(c);
        }
    }
    for (size_t g = primary.size(); g-- > 0;) snapgpu_destroy(primary[g]);
    fprintf(stderr, "snapgpu-sam: %llu reads, %llu mapped records, %d GPU(s) x %d feeder(s), %d formatter thread(s)\n", total, mapped, o.n_gpus, o.ctx_per_gpu, o.n_format);
    if (o.paths.output == Options::DeviceBam || o.paths.output == Options::DeviceBgzf)                     // (the last pass's, like the counts above)
        fprintf(stderr, "snapgpu-sam: BAM records from the device: %llu batches, %llu records\n", g_bam_batches.load(), g_bam_records.load());
    if (o.sorted) {
        fprintf(stderr, "snapgpu-sam: sorted on the device: %llu runs, %llu records, %llu spilled\n", sort_runs, sort_records, sort_spilled);
        if (o.verbose) fprintf(stderr, "snapgpu-sam: merge phase (k-way merge, BGZF on the %s, write): %.3f s\n", merge_on_device ? "device" : "host", s_merge);
    }
    if (o.paths.output == Options::DeviceBgzf)
        fprintf(stderr, "snapgpu-sam: BGZF blocks from the device: %llu batches, %llu blocks, %llu -> %llu bytes\n", g_bgzf_batches.load(), g_bgzf_members.load(),
                g_bgzf_in.load(), g_bgzf_out.load());
    {   // (AlignerContext.cpp:489-543 prints reads/s over the alignment phase, the index load apart: the same split here)
        const double s_stream = pass_s.back();                              // (the last pass; with -passes N each pass printed its own line above)
        fprintf(stderr, "snapgpu-sam: index resident after %.2f s; FASTQ -> %s in %.2f s = %.0f reads/s (%s reader, %d parser thread(s))\n", s_load, o.bam ? "BAM" : "SAM", s_stream,
                s_stream > 0 ? (double)total / s_stream : 0.0, use_map ? "mapped" : "sequential", use_map ? o.n_parse : 1);
        if (o.verbose) {
            fprintf(stderr, "snapgpu-sam: thread-seconds: parse %.2f | feeders: prepare %.2f, align call %.2f, records %.2f, SAM-fields call %.2f | format %.2f | write %.2f\n",
                    g_ns_parse.load() * 1e-9, g_ns_prep.load() * 1e-9, g_ns_align.load() * 1e-9, g_ns_mid.load() * 1e-9, g_ns_samcall.load() * 1e-9, g_ns_format.load() * 1e-9, g_ns_write.load() * 1e-9);
            // the same per THREAD and per PASS: the wall time each stage would take alone with its threads (a stage near the pass's own time is the pipeline's limit)
            const double np = (double)o.passes, nf = (double)fctx.size();
            fprintf(stderr, "snapgpu-sam: waiting, per pass: each feeder %.2f s for parsed batches and %.2f s for room in the formatters' queue; the writer %.2f s for the next batch in order\n",
                    g_ns_wait_in.load() * 1e-9 / np / nf, g_ns_wait_out.load() * 1e-9 / np / nf, g_ns_wait_writer.load() * 1e-9 / np);
            fprintf(stderr, "snapgpu-sam: wall per pass if alone: parse %.2f s (%d threads) | feeders (%d): prepare %.2f, align call %.2f, records %.2f, SAM-fields call %.2f | format %.2f s (%d threads) | write %.2f s (1 thread)\n",
                    g_ns_parse.load() * 1e-9 / np / (use_map ? o.n_parse : 1), use_map ? o.n_parse : 1, (int)fctx.size(), g_ns_prep.load() * 1e-9 / np / nf, g_ns_align.load() * 1e-9 / np / nf,
                    g_ns_mid.load() * 1e-9 / np / nf, g_ns_samcall.load() * 1e-9 / np / nf, g_ns_format.load() * 1e-9 / np / o.n_format, o.n_format, g_ns_write.load() * 1e-9 / np);
        }
    }
    return 0;
}
