/*
 * kmer_api.h — C-ABI of libkmerhip, the MI355X (gfx950) k-mer counter that
 * replaces the FASTQ sliding-window loop of kmerjs (lib/kmers.js).
 *
 * The reference has no native interface; these entry points are what a
 * kmerjs binding (the N-API addon in kmerjs_amd/node/, or ctypes) needs to
 * implement the reference's KmerJS surface unchanged:
 *
 *   reference                                    replaced by
 *   -------------------------------------------  ------------------------------------
 *   new KmerJS(fastq, preffix, length, step, ..) kmer_open(params)        lib/kmers.js:67-82
 *   KmerJS.readFile() -> {promise: Map, event}   kmer_count_file()        lib/kmers.js:106-185
 *     (stream -> liner -> mod-4 -> kmersInLine)  kmer_count_buffer()      lib/kmers.js:114-171
 *   kmersInLine(line), complement(line)          (inside the kernels)     lib/kmers.js:88-100,31-38
 *   Map insertion order / size / entries         kmer_result_*            lib/kmers.js:76,95,177
 *   kmerObj.lines                                kmer_result_lines()      lib/kmers.js:145,165
 *
 * Results are bit-exact with the reference: identical keys (byte strings,
 * including non-ACGT bytes such as N, X, lowercase or '\r'), identical counts,
 * and entries in the reference Map's insertion (first-occurrence) order.
 *
 * Device-resident entry points (kmer_reset / kmer_feed_device /
 * kmer_finish_device) let a caller that already holds the FASTQ bytes in HBM
 * count them without any host copy; kmer_partial_device / kmer_finish_merged
 * merge per-GPU partial results (shards of one input, RCCL over xGMI).
 *
 * Threading: a kmer_ctx is used by one thread at a time (one in-flight call
 * per context); distinct contexts are independent.  All calls return a
 * kmer_status; kmer_last_error() gives a message for the last failure.
 */
#ifndef KMER_API_H
#define KMER_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    KMER_OK = 0,
    KMER_E_IO = 1,            /* file missing/unreadable (reference: uncaught stream error) */
    KMER_E_BAD_PARAM = 2,     /* k == 0, step == 0, NULL pointers, ... */
    KMER_E_OOM = 3,           /* host or device allocation failed */
    KMER_E_DEVICE = 4,        /* HIP runtime error */
    KMER_E_TOO_MANY_KEYS = 5, /* more than max_keys distinct keys (reference: RangeError at 2^24, lib/kmers.js:95) */
    KMER_E_NONASCII = 6,      /* input byte >= 0x80 (reference decodes UTF-8, lib/kmers.js:116) */
    KMER_E_LINE_TOO_LONG = 7, /* a sequence line longer than the order key holds (KMER_FLAG_LONG_LINES) */
    KMER_E_STATE = 8          /* call out of sequence (e.g. finish without reset) */
} kmer_status;

enum {
    KMER_FLAG_TWO_PASS = 1u << 0,  /* debug: exact two-pass line scan instead of single-pass look-back */
    KMER_FLAG_NO_DENSE = 1u << 1,  /* debug: records instead of packed keys (host merge) */
    KMER_FLAG_BYTE_SCAN = 1u << 2, /* debug: byte-SWAR prefix scan instead of the bit-plane scan */
    KMER_FLAG_SORT_FINISH = 1u << 3, /* debug: radix-sort finish instead of the bucket-table finish */
    /* Table mode: the result need not be in Map insertion order.  For step 1,
     * k <= 32 and an empty or A/C/G/T prefix the counts go to a hash-partitioned
     * table of canonical k-mers in HBM (no 2^32-hit session limit; host results
     * sorted by key bytes); other configurations keep the ordered paths. */
    KMER_FLAG_UNORDERED = 1u << 4,
    KMER_FLAG_TABLE_SPLIT_TEST = 1u << 5, /* debug: table mode with 64-key LDS ranges (exercises range splits) */
    /* Canonical k-mers (BASELINE C5; an extension, not the reference's Map):
     * table mode whose result holds one key per {x, rc x} class -- the
     * lexicographically smaller string -- counted once per forward window of
     * the class (jellyfish -C).  Step 1, k <= 32, empty or A/C/G/T prefix
     * (tested on the canonical key); KMER_E_BAD_PARAM otherwise. */
    KMER_FLAG_CANONICAL = 1u << 6,
    /* Long-line mode: order keys with a 40-bit position field, so ordered
     * counts take sequence lines up to 2^40 bytes (FASTA contigs and
     * chromosomes; the reference has no limit, lib/kmers.js:88-100) at up to
     * 2^23 lines.  Default: lines up to 2^23 bytes, 2^40 lines.
     * kmer_count_file / kmer_count_buffer switch to it by themselves when a
     * longer line turns up (the count is redone once); the device-resident
     * calls and multi-GPU group contexts need the flag. */
    KMER_FLAG_LONG_LINES = 1u << 7,
    /* bits 8..15 are reserved (kmer_open rejects them) */
    /* FASTA input (an extension; the reference has no FASTA parser:
     * test/kmers.js:53-61, test/kmerFinderServer.js:158, so its readFile()
     * counts only lines with index % 4 == 1 of a .fsa file, lib/kmers.js:151).
     * A line starting with '>' opens a record (the header is not counted);
     * lines before the first header form a headerless record; a record's
     * sequence is its other lines joined (one trailing '\r' per line dropped),
     * so windows span line breaks; each sequence is counted as the reference
     * counts a sequence line (length > 1; windows of it and of its complement;
     * first-occurrence order by record).  Every mode (ordered, UNORDERED,
     * CANONICAL, any k / step / prefix; records longer than 2^23 bytes through
     * the long-line retry).  kmer_result_lines = input lines.  Device feeds
     * must cut chunks before a header line (offset 0, or a '>' after '\n'). */
    KMER_FLAG_FASTA = 1u << 16,
    /* debug: table pass 1 always with fixed per-workgroup runs (by default
     * only when their filler slots are <= 1/12 of the keys: large inputs), and
     * pass 2 with fixed region capacities at any table size (by default from
     * 2^24 keys) */
    KMER_FLAG_TABLE_FIXED_TEST = 1u << 17,
    /* debug: the general path's first merge attempt reports a hash collision,
     * so the two-hash (h2, h1) retry runs (exercises the collision route) */
    KMER_FLAG_GEN_COLLIDE_TEST = 1u << 18,
    /* debug: the dense-hit path gives every wave 19 consecutive sequence lines
     * at any chunk size (default: ceil(lines / 2^17), i.e. 1 up to 131,072
     * lines per chunk) */
    KMER_FLAG_DENSE_LPW_TEST = 1u << 19
};

typedef struct {
    uint32_t k;               /* kmerLength (reference default 16) */
    uint32_t step;            /* step (reference default 1) */
    const uint8_t *prefix;    /* preffix bytes (reference default "ATGAC"); may be NULL if prefix_len == 0 */
    uint32_t prefix_len;
    int32_t device;           /* HIP device ordinal */
    uint32_t flags;           /* KMER_FLAG_* */
    uint64_t max_keys;        /* 0 = unlimited; 16777216 reproduces the reference Map cap */
    uint64_t batch_bytes;     /* host->device batch size for file/buffer input; 0 = default (files:
                               * 256 MiB, read ahead on a reader thread; buffers: 1 GiB) */
    /* Multi-GPU (SURVEY.md §8b `ndev`): ndev > 1 makes a group context over
     * `devices` (ndev HIP ordinals; NULL = 0..ndev-1; an ordinal may repeat).
     * kmer_count_file / kmer_count_buffer then split the input into ndev
     * line-aligned shards counted concurrently, one per device, and merge the
     * per-device partials (copied to devices[0] over xGMI) into one result in
     * Map order -- bit-exact with a single-device count.  The input is read
     * as a stream of batches cut at '\n' (batch_bytes; default for files
     * 256 MiB, for buffers one share per device) dealt round robin to the
     * devices, so a file never has to fit in host memory.  Table and
     * canonical mode: every device's pass-1 keys go to the device that owns
     * their slice of the hash space, which builds that slice of the table;
     * kmer_table_stats / kmer_table_digest of a group add up its devices'.
     * Every ordered configuration with packed keys is sharded too (any prefix
     * bytes, step > 1).  Only the configurations without packed partials run
     * on devices[0] alone: k > 64 and unprefixed k > 31 (the general path),
     * keys of 64 bits or more (k - |P| >= 32), and KMER_FLAG_NO_DENSE.  A
     * group count that meets a line longer than 2^23 bytes is redone in
     * long-line mode on every device, as a single-device count is.  The other
     * device-resident entry
     * points are single-device only (KMER_E_STATE on a group).  0 or 1 =
     * single device `device`. */
    uint32_t ndev;
    const int32_t *devices;
    /* Progress of kmer_count_file / kmer_count_buffer (replaces the
     * progress-stream of readFile(), lib/kmers.js:108-110): called on the
     * counting thread after each input batch with the input bytes consumed so
     * far and the input's size (for gzip: compressed bytes read and the
     * compressed size).  NULL = none. */
    void (*progress)(void *user, uint64_t done, uint64_t total);
    void *progress_user;
} kmer_params;

typedef struct kmer_ctx kmer_ctx;
typedef struct kmer_result kmer_result;

/* Context lifecycle (replaces `new KmerJS(...)`, lib/kmers.js:67-82). */
kmer_status kmer_open(const kmer_params *params, kmer_ctx **out);
kmer_status kmer_close(kmer_ctx *ctx);

/* Whole-input calls (replace readFile(), lib/kmers.js:106-185). */
/* kmer_count_file also reads gzip-compressed FASTQ (magic 1f 8b) through zlib:
 * the count is that of the decompressed bytes. */
kmer_status kmer_count_file(kmer_ctx *ctx, const char *path, kmer_result **out);
kmer_status kmer_count_buffer(kmer_ctx *ctx, const uint8_t *bytes, size_t len, kmer_result **out);

/* Device-resident streaming: bytes already in HBM.  Each fed chunk must start
 * at a line start (offset 0 of the input, or just after a '\n'); all chunks
 * but the last must end with '\n'.  `stream` is the hipStream_t that produced
 * the bytes (NULL = the legacy default stream): the count waits for the work
 * queued on it so far.  kmer_finish_device leaves the ordered result in
 * device memory (kmer_result_device) and also returns it as a host result
 * when `out` is non-NULL. */
kmer_status kmer_reset(kmer_ctx *ctx);
kmer_status kmer_feed_device(kmer_ctx *ctx, const void *d_bytes, size_t len, void *stream);
kmer_status kmer_finish_device(kmer_ctx *ctx, kmer_result **out);
/* kmer_feed_device returns once the chunk is queued on the context's stream
 * (packed paths); the chunk is settled -- its counters read back, an overflow
 * of the hit lists redone, its errors reported -- by the next call on the
 * context, or explicitly by kmer_sync.  The bytes must stay valid and
 * unchanged until then.  While a chunk is in flight the caller may queue
 * work on other contexts (e.g. another session's finish), which then
 * overlaps the scan on the device.  (lib/kmers.js:148-171 reads the stream
 * chunk by chunk; errors surface at the next call instead of the feed.) */
kmer_status kmer_sync(kmer_ctx *ctx);

/* Multi-GPU merge.  kmer_partial_device reduces this context's session to its
 * unique packed keys: keys = uint64[n] 2-bit suffix codes (the k-|P| bases
 * after the prefix, first base most significant), vals = n x {uint64 first,
 * uint64 count} (first-occurrence order, count).  Keys of 64 bits or more
 * (k - |P| >= 32, counted on the packed path as two words) have no partial:
 * KMER_E_STATE here and in the hit exchange below.  Device pointers, valid until
 * the next call on the context.  Concatenate the partials of every rank on one
 * device (e.g. RCCL gather over xGMI) and hand them to kmer_finish_merged,
 * which reduces again (min first, sum count), orders by first occurrence and
 * decodes.  Record keys (non-ACGT windows) stay on the host: move them with
 * kmer_records_export / kmer_records_import.  KMER_E_STATE when the
 * configuration has no packed keys. */
kmer_status kmer_partial_device(kmer_ctx *ctx, const void **d_keys, const void **d_vals, uint64_t *n);
kmer_status kmer_finish_merged(kmer_ctx *ctx, const void *d_keys, const void *d_vals, uint64_t n,
                               uint64_t total_lines, kmer_result **out);
/* Multi-GPU hit exchange (the default multi-GPU finish).  After the feeds,
 * kmer_exchange_prepare partitions this session's counting hits by owning
 * rank -- equal slices of the packed-key space over `world` ranks (world <=
 * 256) -- into d_send: per owner a contiguous run of 16-byte records {uint64
 * first-occurrence order key, uint64 packed key}, runs in owner order, each
 * run in first-occurrence order; counts[o] (host array of `world`) = records
 * for owner o.  d_send is valid until the next call on the context.  Exchange
 * the runs (all-to-all over xGMI) and hand each rank's received records,
 * concatenated in source-rank order, to kmer_finish_exchanged, which counts
 * them (this rank's key range of the result, in first-occurrence order,
 * device-resident: kmer_result_device).  `wait_stream` (hipStream_t; NULL =
 * the legacy default stream): the context's stream waits for the work queued
 * so far on that stream (the collective that wrote d_recv) before reading it.  Shards must be fed in
 * line order (kmer_set_position) so that order keys are global. */
kmer_status kmer_exchange_prepare(kmer_ctx *ctx, uint32_t world, const void **d_send, uint64_t *counts);
kmer_status kmer_finish_exchanged(kmer_ctx *ctx, const void *d_recv, uint64_t n, uint64_t total_lines,
                                  void *wait_stream, kmer_result **out);
/* One result in Map order from every rank's ordered key range (the device
 * result of kmer_finish_exchanged on each rank), gathered to this context's
 * device and concatenated (any order): n rows of keys (n * k bytes), counts
 * (uint64) and first-occurrence keys (uint64).  Re-orders them by first
 * occurrence into this context's device result (kmer_result_device) and,
 * when `out` is non-NULL, returns the host result with this context's record
 * keys merged in (import the other ranks' records first). */
kmer_status kmer_merge_ordered(kmer_ctx *ctx, const void *d_keys, const void *d_counts, const void *d_firsts,
                               uint64_t n, uint64_t total_lines, kmer_result **out);
kmer_status kmer_records_export(kmer_ctx *ctx, kmer_result **out);
kmer_status kmer_records_import(kmer_ctx *ctx, const char *keys, const uint64_t *offsets,
                                const uint64_t *counts, const uint64_t *firsts, uint64_t n);
/* Drop this session's record keys (after they were moved to another rank). */
kmer_status kmer_records_clear(kmer_ctx *ctx);
/* Ordered result of the last finish, still in device memory (packed path):
 * keys = n * k bytes, counts = uint64[n], firsts = uint64[n]. */
kmer_status kmer_result_device(kmer_ctx *ctx, const void **d_keys, const void **d_counts,
                               const void **d_firsts, uint64_t *n);
/* Set the running line/byte position (lines already consumed, absolute byte
 * offset of the next fed chunk) — used when one input is sharded over ranks. */
kmer_status kmer_set_position(kmer_ctx *ctx, uint64_t lines_before, uint64_t byte_offset);
/* Lines consumed so far (reference kmerObj.lines). */
kmer_status kmer_lines(kmer_ctx *ctx, uint64_t *lines);

/* Ordered result (Map insertion order). */
uint64_t kmer_result_size(const kmer_result *r);
uint64_t kmer_result_lines(const kmer_result *r);
kmer_status kmer_result_get(const kmer_result *r, uint64_t i, const char **key, uint32_t *klen,
                            uint64_t *count);
/* Bulk view: keys packed back to back; key i = keys[offsets[i] .. offsets[i+1]). */
kmer_status kmer_result_arrays(const kmer_result *r, const char **keys, const uint64_t **offsets,
                               const uint64_t **counts);
/* First-occurrence order key of every entry (monotone in Map order). */
kmer_status kmer_result_firsts(const kmer_result *r, const uint64_t **firsts);
/* Write a result to a file, in Map order: KMER_WRITE_JSON = JSON.stringify of
 * mapToJSON(map) (lib/kmers.js:46-54); KMER_WRITE_LEGACY = the npm main's
 * "{\n key: count, ... }\n" dump (lib/index.js:381-388). */
enum { KMER_WRITE_JSON = 0, KMER_WRITE_LEGACY = 1 };
kmer_status kmer_result_write(const kmer_result *r, const char *path, uint32_t format);
void kmer_result_free(kmer_result *r);

/* Benchmark utility: write n_reads synthetic 317-byte FASTQ records (SURVEY.md
 * §8d generator, splitmix64 of (seed, read index)) to device memory. */
kmer_status kmer_synth_fastq_device(void *d_out, uint64_t seed, uint64_t first_read, uint64_t n_reads,
                                    void *stream);

/* Table mode (KMER_FLAG_UNORDERED), after a finish.  The counts replace the
 * reference Map (lib/kmers.js:95) when it would be too large to build:
 *   canonical = distinct canonical k-mers in the table,
 *   keys      = distinct Map keys (both orientations, prefix-filtered, + records),
 *   total     = sum of the Map's counts (= counted windows on both strands). */
kmer_status kmer_table_stats(kmer_ctx *ctx, uint64_t *canonical, uint64_t *keys, uint64_t *total);
/* Batched lookup against the table (after a finish): the Map's `get` for n
 * query keys of exactly k bytes each, back to back; counts[i] (uint64) = the
 * value of key i in the Map this context's host result describes
 * (kmer_count_buffer / kmer_finish_device(.., out)), 0 when the key is not in
 * it.  For an A/C/G/T key x with C[.] the table's count of a class {x, rc x}:
 * table mode -- 0 unless x starts with the prefix, else C[class of x], doubled
 * when x is its own reverse complement; canonical mode -- 0 unless x is the
 * lexicographically smaller of {x, rc x} and starts with the prefix, else
 * C[class of x].  Keys with any other byte (N, lowercase, '\r', ...) are record
 * keys, which live on the host: kmer_table_lookup answers them from the
 * context's records (as the host result lists them), kmer_table_lookup_device
 * answers 0 for them.  The lookup runs on the device against the table where
 * it lies and leaves it unchanged; it may be repeated, and interleaved with
 * kmer_table_stats / kmer_table_digest, until the next reset.  An exchanged
 * table (kmer_table_finish_exchanged) answers 0 for classes other ranks own,
 * so the ranks' answers add up.
 * kmer_table_lookup: host arrays; the keys go up in bounded pieces, so device
 * and pinned memory do not grow with n.  On a group (ndev > 1) every child
 * looks all keys up in its slice of the table and the answers add.
 * kmer_table_lookup_device: d_keys (n * k bytes) and d_counts (n uint64) in
 * device memory, single-device contexts only (KMER_E_STATE on a group); the
 * lookup waits for the work queued so far on `stream` (hipStream_t; NULL = the
 * legacy default stream), and d_counts is complete when the call returns.
 * KMER_E_STATE unless a table finish holds results; KMER_E_BAD_PARAM for NULL
 * pointers with n > 0; n == 0 is KMER_OK and touches nothing. */
kmer_status kmer_table_lookup(kmer_ctx *ctx, const char *keys, uint64_t n, uint64_t *counts);
kmer_status kmer_table_lookup_device(kmer_ctx *ctx, const void *d_keys, uint64_t n, void *d_counts, void *stream);
/* Reads screened against the table (after a table finish, until the next
 * reset; the calls may be repeated and interleaved with stats, digest, lookup,
 * spectrum, extract, setops and match, and leave the table, its bucket index,
 * the big list, kmer_lines, the context's records and the session's position
 * unchanged).  Input is FASTQ bytes: lines are '\n'-separated, line i runs up
 * to the (i+1)-th '\n' or to the end of the bytes, and the reads are the lines
 * with i % 4 == 1 and i <= the number of '\n' (data.split("\n")[1::4]); the
 * line finder works from line phase 0 in every call.  Read r gets one row, in
 * input order.  "T" is the Map this context's host result describes, the one
 * kmer_table_lookup answers for; the read's own Map is the one the same
 * configuration (k, prefix, mode) builds from a file holding that record alone:
 *   windows = the sum of the own Map's values over its A/C/G/T keys,
 *   hits    = that sum restricted to keys x with T(x) >= max(min_count, 1),
 *   sum     = the sum of own(x) * T(x), mod 2^64, over the same keys,
 *   skipped = the read's forward windows that hold a byte outside A/C/G/T
 *             (record keys, which live on the host and are not matched).
 * A line of 0 or 1 bytes gives a zero row (the count ignores it,
 * lib/kmers.js:151).  Per forward window w of a counted line, with C the
 * table's count of its class {w, rc w} (0 when absent; a 0xFFFFF count field
 * resolves through the big list): table mode -- f = "w starts with the
 * prefix", r = "rc w starts with it"; w != rc w: weight m = f + r, value v = C;
 * w == rc w: m = 2 f, v = 2 C.  Canonical mode -- m = "the smaller string of
 * the class starts with the prefix", v = C.  Then windows += m and, if v >=
 * max(min_count, 1), hits += m and sum += m v.  One probe per forward window,
 * by class.  An exchanged table answers 0 for classes other ranks own: hits
 * and sum add up over ranks, windows and skipped are equal on every rank.
 *
 * kmer_table_screen_device: the bytes are in device memory, start at a record
 * start, may end without '\n' and may sit at any byte alignment; nothing
 * outside [d_bytes, d_bytes + len) is loaded.  The call waits for the work
 * queued so far on `stream` (as the lookup does); *d_rows = *n_reads rows of
 * kmer_read_screen, library-owned device memory, complete when the call
 * returns and valid until the next screen, reset or close (not the extract's
 * buffers, which stay valid).  A chunk in flight is settled first.
 * kmer_table_screen: host bytes; they go up in bounded pieces cut at record
 * boundaries (batch_bytes, default 64 MiB), so device and pinned memory do not
 * grow with len.  At most cap rows are written; *n_reads is always the true
 * number, and cap < *n_reads is KMER_E_BAD_PARAM with *n_reads set.
 *
 * flags (of the call; kmer_open's flags are not involved): 0 = auto -- the
 * sorted route when the table's entries divided by the buckets it owns exceed
 * KMER_SCREEN_DIRECT_MAX, else the direct one.  KMER_SCREEN_DIRECT: windows
 * are probed in input order, a bucket is scanned per window.
 * KMER_SCREEN_SORTED: the windows of a piece are sorted by bucket first, and a
 * long bucket is read once per run of windows.  Both, or an unknown bit:
 * KMER_E_BAD_PARAM.  KMER_SCREEN_PIECE_TEST (debug): internal pieces of 4,096
 * windows instead of 2^26, so lines are cut across pieces.
 *
 * Checked before any device call: KMER_E_BAD_PARAM for a NULL context or
 * out-pointer, NULL bytes with len > 0, or bad flags; len == 0 is KMER_OK with
 * *n_reads = 0 and touches nothing; KMER_E_STATE for a group context (ndev >
 * 1), a context not in table mode or without a table finish, or a
 * KMER_FLAG_FASTA context.  KMER_E_NONASCII as for a feed (the table stays
 * readable); KMER_E_OOM leaves the context usable; KMER_E_DEVICE, naming the
 * bucket, if a bucket's extent lies past the table (it is not read). */
typedef struct {
    uint64_t windows, hits, skipped, sum;
} kmer_read_screen;
enum { KMER_SCREEN_DIRECT = 1u, KMER_SCREEN_SORTED = 2u, KMER_SCREEN_PIECE_TEST = 4u };
#define KMER_SCREEN_DIRECT_MAX 16u /* mean entries per owned bucket up to which auto picks DIRECT */
kmer_status kmer_table_screen_device(kmer_ctx *ctx, const void *d_bytes, size_t len, uint64_t min_count,
                                     uint32_t flags, void *stream, const void **d_rows, uint64_t *n_reads);
kmer_status kmer_table_screen(kmer_ctx *ctx, const uint8_t *bytes, size_t len, uint64_t min_count,
                              uint32_t flags, kmer_read_screen *rows, uint64_t cap, uint64_t *n_reads);
/* Reads filtered by their screen (after a table finish, until the next reset):
 * the screen above, then the records of the reads that pass a predicate on
 * their rows, compacted on the device.  Input is FASTQ bytes under exactly the
 * screen's rules (lines, reads, n_reads, line phase 0 in every call).
 *   Records:  record r (0 <= r < n_reads) is the bytes from the start of line
 *             4r up to and including the '\n' that ends line 4r + 3; when the
 *             input has no such '\n' the record runs to the end of the input.
 *             Records are back to back from offset 0.
 *   consumed: the end of record n_reads - 1, or 0 when there is no read.
 *   The tail: len - consumed bytes may remain -- an unfinished header line
 *             after a complete record, or an input without any '\n'.  They
 *             hold no read and are never part of the output; a streaming
 *             caller carries them into the next call.
 *   row(r):   the screen's row of read r at the call's min_count.
 *   match(r): hits >= min_hits AND hits * frac_den >= frac_num * windows, in
 *             exact (128-bit) arithmetic.  With min_hits = 0 and frac_num = 0
 *             every read matches, also one without windows.
 *   KMER_FILTER_PAIRED: records 2j and 2j + 1 are mates (interleaved pairs);
 *             both get match(2j) OR match(2j + 1).  A last record without a
 *             mate is judged alone.
 *   keep(r):  match(r), negated under KMER_FILTER_DROP.
 *   Output:   the kept records, verbatim and in input order, back to back.  No
 *             byte is added: only the input's last record can lack its final
 *             '\n', and it is then last in the output too.
 *
 * kmer_table_filter_device: the screen's preconditions and guarantees -- the
 * bytes are in device memory, start at a record start and sit at any byte
 * alignment; nothing outside [d_bytes, d_bytes + len) is loaded; the call
 * waits for the work queued so far on `stream`, is complete on return, and a
 * chunk in flight is settled first.  *d_out = out_len bytes, *d_keep = n_reads
 * bytes of 0 / 1, *d_rows = the screen's n_reads rows: library-owned device
 * memory, valid until the next screen, filter, reset or close.  The rows share
 * the screen's buffer, so a filter ends the validity of an earlier screen's
 * rows (and a screen that of a filter's three outputs).  Any of the three
 * out-pointers may be NULL (NULL d_out: the records are not copied); one whose
 * array is empty is set to NULL.  The extract's buffers stay valid.
 * kmer_table_filter: host bytes; they go up in bounded pieces cut at record
 * boundaries as in kmer_table_screen (under KMER_FILTER_PAIRED at pair
 * boundaries, so mates are never split), and each piece's output and flags
 * come down before the next piece goes up: device and pinned memory do not
 * grow with len.  out == NULL with out_cap == 0 returns counts and flags only,
 * and likewise keep; out_cap >= len always suffices, keep_cap >= n_reads is
 * needed; a buffer that turns out too small is KMER_E_BAD_PARAM with a message
 * naming both sizes (what was written before is unspecified).
 *
 * Checked before any device call: KMER_E_BAD_PARAM for a NULL context, p or
 * res, NULL bytes with len > 0, frac_den == 0 or frac_num > frac_den, an
 * unknown bit in flags, or the screen's own flag errors in screen_flags; len
 * == 0 is KMER_OK with a zero result and touches nothing.  KMER_E_STATE,
 * KMER_E_NONASCII, KMER_E_OOM and KMER_E_DEVICE exactly as in the screen: the
 * table stays readable and the context usable.  The call leaves unchanged what
 * the screen leaves unchanged. */
enum { KMER_FILTER_DROP = 1u, KMER_FILTER_PAIRED = 2u };
typedef struct {
    uint64_t min_count;           /* the screen's */
    uint64_t min_hits;
    uint32_t frac_num, frac_den;  /* frac_den >= 1, frac_num <= frac_den */
    uint32_t flags;               /* KMER_FILTER_* */
    uint32_t screen_flags;        /* KMER_SCREEN_* of the underlying screen */
} kmer_filter_params;             /* 32 bytes */
typedef struct {
    uint64_t n_reads, n_kept, out_len, consumed;
} kmer_filter_result;
kmer_status kmer_table_filter_device(kmer_ctx *ctx, const void *d_bytes, size_t len, const kmer_filter_params *p,
                                     void *stream, const void **d_out, const void **d_keep, const void **d_rows,
                                     kmer_filter_result *res);
kmer_status kmer_table_filter(kmer_ctx *ctx, const uint8_t *bytes, size_t len, const kmer_filter_params *p,
                              uint8_t *out, uint64_t out_cap, uint8_t *keep, uint64_t keep_cap,
                              kmer_filter_result *res);
/* The table read by value (after a table finish, until the next reset; the
 * calls may be repeated and interleaved with stats, digest, lookup and match,
 * and leave the table unchanged).  "The Map" is the Map this context's host
 * result describes, the one kmer_table_lookup answers for.  A table entry is a
 * class {x, rc x} with count C.  Table mode: key x with value C if x starts
 * with the prefix, key rc x likewise; when x == rc x, one key with value 2 C.
 * Canonical mode: one key, the smaller string of the class, value C, if it
 * starts with the prefix.  Record keys (a byte outside A/C/G/T) live on the
 * host and are counted by the host-returning calls only, as kmer_table_stats
 * counts them.
 *
 * kmer_table_spectrum: the abundance spectrum (jellyfish histo).  hist = a
 * host array of nbins uint64, 2 <= nbins <= KMER_SPECTRUM_MAX_BINS
 * (KMER_E_BAD_PARAM otherwise); every Map key of value v adds 1 to
 * hist[min(v, nbins - 1)], hist[0] = 0, and *top_sum (may be NULL) = the sum
 * of the values of the keys in the last bin.  With (canonical, keys, total) of
 * kmer_table_stats: sum hist = keys, and sum of v hist[v] over v < nbins - 1,
 * plus top_sum, = total.  A group adds its children's histograms; the
 * histograms of the ranks of an exchanged table add up.  The kernel keeps
 * values up to KMER_SPECTRUM_REG_MAX in registers and values below
 * KMER_SPECTRUM_LDS_BINS in LDS; the rest are global atomics.
 *
 * kmer_table_extract_device: the A/C/G/T Map keys with lo <= value <= hi
 * (hi == 0: no upper bound; lo == 0 is 1; hi != 0 && hi < lo: n = 0), sorted
 * ascending by key bytes: *d_keys = n * k key bytes back to back, *d_counts =
 * n uint64 values, library-owned device memory that is complete when the call
 * returns and valid until the next extract, reset or close on the context
 * (kmer_match_open_device takes them as they are).  Single-device contexts
 * only (KMER_E_STATE on a group); an exchanged table extracts its own share.
 * The buffers are sized from a counting pass; KMER_E_OOM leaves the context
 * usable.
 *
 * kmer_table_extract: the rows of the context's host result whose value is in
 * range, in the same order (by key bytes, record keys included), computed
 * through the device extract: only the qualifying keys are copied to the
 * host.  On a group the children's extracts are merged by key.
 *
 * KMER_E_STATE unless a table finish holds results; KMER_E_BAD_PARAM for NULL
 * out-pointers; KMER_E_DEVICE, naming the bucket, if a bucket's extent lies
 * past the table (it is not read). */
#define KMER_SPECTRUM_REG_MAX 4u
#define KMER_SPECTRUM_LDS_BINS 4096u
#define KMER_SPECTRUM_MAX_BINS (1u << 21)
kmer_status kmer_table_spectrum(kmer_ctx *ctx, uint32_t nbins, uint64_t *hist, uint64_t *top_sum);
kmer_status kmer_table_extract_device(kmer_ctx *ctx, uint64_t lo, uint64_t hi, const void **d_keys,
                                      const void **d_counts, uint64_t *n);
kmer_status kmer_table_extract(kmer_ctx *ctx, uint64_t lo, uint64_t hi, kmer_result **out);
/* Two tables related to each other (both after a table finish, until the next
 * reset of either; the calls may be repeated and interleaved with stats,
 * digest, lookup, spectrum, extract and match, and leave both tables
 * unchanged).  "The Map of A" is the Map context a's host result describes,
 * as above; a key is IN A iff its value there is >= max(min_a, 1), IN B
 * likewise with min_b.  The two contexts have the same k, mode and prefix, so
 * a class {x, rc x} has the same Map keys (and the same doubling) on both
 * sides: the tables are joined on the class, bucket by bucket (equal k: equal
 * hash, bucket q of A meets bucket q of B only), on the device in LDS.  A
 * count field of 0xFFFFF resolves through that side's big list.  a == b is
 * legal.
 *
 * KMER_JOIN_TILE: the entries of one bucket a wave stages in LDS at a time (a
 * longer bucket is split by leading remainder bits and both sides are re-read
 * per part).
 *
 * kmer_table_overlap: keys_a / keys_b = the distinct Map keys in A / in B,
 * keys_both = the keys in both; total_a / total_b = the sum of the values of
 * the keys in A / in B; shared_a / shared_b = the sum of A's / of B's values
 * over the keys in both; sum_min = the sum of min(vA, vB) over the keys in
 * both.  (Jaccard = keys_both / (keys_a + keys_b - keys_both), containment of
 * A = keys_both / keys_a, Bray-Curtis = 1 - 2 sum_min / (total_a + total_b).)
 *
 * kmer_table_compare: *out filled, record keys (a byte outside A/C/G/T; they
 * live on the host) included as kmer_table_stats includes them: with min_a =
 * min_b = 1, keys_a and total_a are the keys and total of kmer_table_stats(a),
 * keys_b and total_b those of b.  The ranks' structs of two tables exchanged
 * with the same world and rank add up.
 *
 * KMER_SETOP_*: INTERSECT = the keys in A and in B, value min(vA, vB);
 * SUBTRACT = the keys in A and not in B, value vA; UNION = the keys in A or
 * in B, value = the sum of the values of the sides the key is in.
 *
 * kmer_table_setop_device: the A/C/G/T keys of the operation's result sorted
 * ascending by key bytes: *d_keys = n * k key bytes back to back, *d_counts =
 * n uint64 values, library-owned device memory of context a (the extract's
 * buffers), complete when the call returns and valid until the next extract,
 * setop, reset or close on a (kmer_match_open_device takes them as they are).
 * The buffers are sized from a counting pass; KMER_E_OOM leaves both contexts
 * usable.  Exchanged tables (same world and rank) give their share: the
 * ranks' results are disjoint.
 *
 * kmer_table_setop: the host twin, a result in the host result's order (by
 * key bytes), with the record keys of the two contexts joined by the same
 * rules and merged in; its lines are those of a.
 *
 * The work runs on a's stream, which waits for the work queued on b's; a
 * chunk in flight on either context is settled first.  The call uses both
 * contexts: neither may be in use on another thread.  Checked before any
 * device call: KMER_E_BAD_PARAM for NULL contexts or out-pointers, op >
 * KMER_SETOP_UNION, contexts on different devices, or contexts that differ in
 * k, KMER_FLAG_CANONICAL or prefix bytes; KMER_E_STATE for a group context
 * (ndev > 1), a context not in table mode, or one without a table finish.
 * KMER_E_DEVICE, naming the bucket and the context, if a bucket's extent lies
 * past its table (it is not read).
 *
 * kmer_table_setop_into: the same operation (a, b, op, min_a, min_b exactly as
 * above, a == b legal) with a table as its result, so that operations chain,
 * counts of separate sessions merge (UNION, as `jellyfish merge`), and reads
 * are screened or filtered against "A minus B".  dst is a third context:
 * single-device, in table mode, on the same device, equal to a in k,
 * KMER_FLAG_CANONICAL and prefix bytes, in any session state (a chunk in
 * flight is settled, then dst is reset as by kmer_reset).  After KMER_OK dst
 * is in the state a table finish leaves, until its next reset: stats, digest,
 * lookup, spectrum, extract, screen, filter, kmer_table_device,
 * kmer_match_open_table, compare and the setops (dst as a, b or, in a later
 * call, dst again) work on it.  The Map dst describes -- the one its lookup
 * answers for and kmer_table_extract(dst, 1, 0) lists -- equals row for row
 * the host result of kmer_table_setop(a, b, op, min_a, min_b): the record keys
 * of a and b, joined on the host by the same rules, become dst's records;
 * kmer_lines(dst) is a's.  kmer_table_stats(dst) and kmer_table_digest(dst)
 * are those of a count that produced this Map; with thresholds 1,
 * digest(UNION) = digest(a) + digest(b) mod 2^64, and the UNION of the tables
 * of inputs X and Y has the stats, digest and lookup answers of one count
 * over X followed by Y.  The operation on the Map values is the operation on
 * the class counts (both sides double a self-complementary key alike), the
 * threshold tested on the Map value; a class without a Map key (canonical
 * mode, a prefix only its larger string starts with) has its class count for
 * a value.  The result's entry is remainder << 20 | min(C, 0xFFFFF); a count C
 * >= 0xFFFFF -- a UNION can make one from two small ones -- goes to dst's big
 * list; a result of 0 is no entry.  Bucket q of the result is written
 * straight from the join of bucket q of a and b (entries per bucket counted,
 * scanned, then written; the order within a bucket is unspecified): no sort
 * and no decode to key bytes, and dst's entries, bucket index and big list are
 * allocated exactly.  a and b are left unchanged: table, bucket index, big
 * list, records, kmer_lines, and (unlike kmer_table_setop_device) a's extract
 * buffers.  Exchanged a and b (same world and rank) give dst that rank's
 * share: the ranks' stats and digests of dst add up.
 * The work runs on dst's stream, which waits for the work queued on a's and
 * b's; the call is complete on return, and none of the three contexts may be
 * in use on another thread.  Checked before any device call: KMER_E_BAD_PARAM
 * for a NULL context, op > KMER_SETOP_UNION, dst == a or dst == b (no in-place
 * operation), contexts on different devices, dst or b differing from a in k,
 * KMER_FLAG_CANONICAL or prefix bytes; KMER_E_STATE for a group context among
 * the three, a or b not in table mode or without a table finish, dst not in
 * table mode.  During the call: KMER_E_OOM leaves all three contexts usable,
 * dst in its reset state; KMER_E_DEVICE names the bucket and the context, as
 * above.  The message of a failure is a's last error. */
#define KMER_JOIN_TILE 1024u
typedef struct {
    uint64_t keys_a, keys_b, keys_both;   /* distinct Map keys in A, in B, in both            */
    uint64_t total_a, total_b;            /* sum of their values                              */
    uint64_t shared_a, shared_b;          /* sum of A's / of B's values over the keys in both */
    uint64_t sum_min;                     /* sum of min(vA, vB) over the keys in both         */
} kmer_table_overlap;
kmer_status kmer_table_compare(kmer_ctx *a, kmer_ctx *b, uint64_t min_a, uint64_t min_b, kmer_table_overlap *out);
enum { KMER_SETOP_INTERSECT = 0, KMER_SETOP_SUBTRACT = 1, KMER_SETOP_UNION = 2 };
kmer_status kmer_table_setop_device(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b,
                                    const void **d_keys, const void **d_counts, uint64_t *n);
kmer_status kmer_table_setop(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b,
                             kmer_result **out);
kmer_status kmer_table_setop_into(kmer_ctx *a, kmer_ctx *b, uint32_t op, uint64_t min_a, uint64_t min_b,
                                  kmer_ctx *dst);
/* The table itself, in device memory (to read counts, use kmer_table_lookup,
 * which owns the two key encodings below; this is the raw layout for a
 * consumer that walks the whole table; the library's own are
 * kmer_table_spectrum and kmer_table_extract).  2^20 buckets; bucket q holds
 * bucket_len[q] (uint32) entries at entries[bucket_start[q] ..] (uint64 each:
 * remainder << 20 | count, count == 0xFFFFF meaning "see the big list").
 * h = q << 44 | remainder = c * 0x9E3779B97F4A7C15 (mod 2^64), a bijection of the canonical
 * planar code c = min(code(w), code(rc w)) with code = hi_plane << k | lo_plane,
 * base i of the k-mer at bit i of each plane, A/C/G/T = (hi,lo) 00/01/10/11.
 * k <= 21 (narrow keys): h = f(c') << 23, f(x) = (x ^ (x >> 21)) *
 * 0x9E3779B97F4A7C15 mod 2^41 (the remainder's low 23 bits are 0), where c'
 * is, for even k, c; for odd k, the planar code of the orientation (w or
 * rc w) whose middle base is A or C, with that base's high-plane bit (bit
 * k + (k - 1) / 2, zero) taken out.  Inverse: x = z ^ (z >> 21), z = (h >>
 * 23) * 0x9E3779B97F4A7C15^-1 mod 2^41, then (odd k) a zero bit put back at
 * k + (k - 1) / 2.  (The digest weighs c * 0x9E3779B97F4A7C15 for every k.)
 * big = n_big {uint64 h, uint64 count} pairs.  Valid until the next reset. */
kmer_status kmer_table_device(kmer_ctx *ctx, const void **d_entries, const void **d_bucket_start,
                              const void **d_bucket_len, const void **d_big, uint64_t *n_big);
/* Linear digest of the table (after a finish): sum over its canonical entries
 * of count x mix(h) mod 2^64, mix = the splitmix64 finalizer
 * (z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB;
 * z ^= z >> 31).  Linear in the counts: the digest of a count over input
 * A + B is the sum of the digests over A and over B, and the ranks' digests
 * of an exchanged table add up -- a size-independent check of a table that is
 * too large to compare entry by entry.  Record keys are not included. */
kmer_status kmer_table_digest(kmer_ctx *ctx, uint64_t *digest);
/* Diagnostics of table mode's routes since the last reset.  Pass 1: chunks
 * whose keys went out in fixed-capacity runs (p1_fixed), of them the chunks
 * whose workgroup shares were merged first (p1_merged: small shares, e.g. long
 * contigs cut into pieces), and chunks counted by the two-pass route
 * (p1_counted).  Pass 2: finishes that ran with fixed bucket capacities and no
 * histogram pass (p2_fixed: large buckets).  Lets a test assert which route a
 * workload took. */
kmer_status kmer_table_routes(kmer_ctx *ctx, uint64_t *p1_fixed, uint64_t *p1_merged, uint64_t *p1_counted,
                              uint64_t *p2_fixed);
/* Diagnostics of the dense-hit path (a 1-3-base A/C/G/T prefix, step 1,
 * k <= 64) since the last reset: the chunks that went through it and the
 * largest number of consecutive sequence lines a wave was given in any of
 * them (0 when there was none).  Either pointer may be NULL.  A context on
 * another path answers KMER_OK with zeros; a group context KMER_E_STATE.  Lets
 * a test assert that its waves took several lines. */
kmer_status kmer_dense_routes(kmer_ctx *ctx, uint64_t *chunks, uint64_t *lines_per_wave);
/* Table mode across ranks (replaces the one Map.set stream of lib/kmers.js:95
 * when the count is sharded over GPUs; reads are independent, :151-155).
 * Rank o (of `world` <= 1024) owns the pass-1 partitions [o*1024/world,
 * (o+1)*1024/world) -- a contiguous slice of the hash space h and its
 * buckets.  After the feeds, kmer_table_exchange_prepare returns in d_send,
 * per owner, a contiguous run of uint64 pass-1 keys (runs in owner order, each
 * partition-major); counts[o] (host, `world`) = keys for owner o; parts[p]
 * (host, 1024) = this session's keys per partition.  d_send is valid until the
 * next call on the context.  Exchange the runs (all-to-all over xGMI) and the
 * parts tables (all-gather), then hand the received runs, concatenated in
 * source-rank order (n keys), and parts (world x 1024, source-rank order) to
 * kmer_table_finish_exchanged: pass 2 + final over this rank's buckets
 * (others empty).  The table is written over d_recv, which must stay alive
 * until the next reset; kmer_table_stats / kmer_table_device then describe
 * this rank's share (the ranks' stats add up: partitions are disjoint; move
 * record keys to one rank first, kmer_records_export / _import / _clear).
 * `wait_stream` as for kmer_finish_exchanged. */
kmer_status kmer_table_exchange_prepare(kmer_ctx *ctx, uint32_t world, const void **d_send, uint64_t *counts,
                                        uint64_t *parts);
kmer_status kmer_table_finish_exchanged(kmer_ctx *ctx, void *d_recv, uint64_t n, const uint64_t *parts,
                                        uint32_t world, uint32_t rank, void *wait_stream);

/* Device time (HIP events on the context's stream, ms) since the last reset:
 * scan_ms = the streaming tile-scan kernel(s) alone, feed_ms = every kernel of
 * the feeds (scan + line scans + hit resolution), finish_ms = the last finish
 * (compaction + sort + decode).  Waits for the last finish only when
 * finish_ms is non-NULL. */
kmer_status kmer_last_timing(kmer_ctx *ctx, double *scan_ms, double *feed_ms, double *finish_ms);

/* Device time per phase since the last reset (HIP events on the context's
 * stream, ms; feeds summed).  Table mode: "lines" (newline array, sequence
 * lines), "hist1" (+ its scan), "scatter1", "hist2" (+ scan), "scatter2",
 * "final"; ordered modes: "scan", "feed", "finish" as kmer_last_timing.
 * Up to `max` entries are written; *n = the number of phases. */
kmer_status kmer_phase_times(kmer_ctx *ctx, uint32_t max, const char **names, double *ms, uint32_t *n);

const char *kmer_status_string(kmer_status s);
const char *kmer_last_error(const kmer_ctx *ctx);
const char *kmer_version(void);

#ifdef __cplusplus
}
#endif
#endif /* KMER_API_H */
