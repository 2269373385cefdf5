/*
 * kmer_match.h — C-ABI of the k-mer -> template matcher in libkmerhip
 * (SURVEY.md §8f row 3): kmerFinder's hash-join of a query k-mer Map against
 * a template database, on the GPU.
 *
 *   reference                                             replaced by
 *   ----------------------------------------------------  ---------------------------
 *   Redis kmer -> [template] lists, Mongo `reads`         kmer_db_open
 *     (src/kmerPyToMongo.py:21-42)
 *   the ETL itself: genomes -> each template's k-mer      kmer_db_open_fasta
 *     set, `lengths`, `ulength`, names                    (+ kmer_db_template_stats / _kmers / _name)
 *     (src/kmerPyToMongo.py, offline, over pickles)
 *   findKmersMatchesRedis: one lrange per query k-mer,    kmer_match_open
 *     templates scored in first-hit order                 (+ kmer_match_templates)
 *     (lib/kmerFinderServer.js:171-226)
 *   the same with a Map too large to build (2^24 keys):   kmer_match_open_table
 *     the query stays in the counter's device table       (+ kmer_db_kmers)
 *   findWinner: templates sorted by uScore, first wins    kmer_match_winner
 *     (:741-752, sortKmerMatches :700-709)
 *   removeWinnerKmers + getMatches: the winner's k-mers   kmer_match_remove
 *     leave the query, every template is re-scored
 *     (:778-830)
 *   findMatchesMongoAggregation: templates in DB order    kmer_match_templates(.., DB order)
 *     (:452-522)
 *
 * The statistics of a winner (lib/stats.js zScore / fastp, matchSummary
 * lib/kmerFinderServer.js:625-676, bignumber.js decimals) are scalar host work
 * done by the caller (kmerjs_amd/node/kmerfinder.js, kmerjs_amd/kmerfinder.py)
 * between kmer_match_winner and kmer_match_remove.
 *
 * K-mers are byte strings of length k <= 32 over A/C/G/T (upper case).  A
 * query key of another length or with another byte never matches (the
 * reference compares strings).  Within one k-mer's template list, templates
 * are in ascending DB order; a template's duplicate k-mers count once
 * (the ETL's list(set(...)), src/kmerPyToMongo.py:23).
 */
#ifndef KMER_MATCH_H
#define KMER_MATCH_H

#include <stddef.h>
#include <stdint.h>

#include "kmer_api.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kmer_db kmer_db;
typedef struct kmer_match kmer_match;

/* Template DB on `device`: n_keys k-mers (keys = n_keys * k bytes back to
 * back); template t owns keys [template_start[t], template_start[t + 1]),
 * template_start has n_templates + 1 entries (0 ... n_keys).
 * KMER_E_BAD_PARAM for k == 0 or k > 32, a byte outside A/C/G/T, or bad
 * offsets. */
kmer_status kmer_db_open(int32_t device, uint32_t k, const char *keys, uint64_t n_keys,
                         const uint64_t *template_start, uint32_t n_templates, kmer_db **out);
/* Template DB straight from FASTA genomes, built on the device of `ctx` (the
 * replacement of the offline ETL).  The input is FASTA under the rules of
 * KMER_FLAG_FASTA (kmer_api.h: header lines, a headerless first record, lines
 * joined, one trailing '\r' per line dropped, empty lines add nothing, a
 * sequence of length <= 1 is not counted), whether or not the context has that
 * flag.  Record r of the input, in input order, is template r -- records
 * without k-mers included, so template indices are record ordinals.  The
 * k-mers of template r are the A/C/G/T keys of the record's own Map: the Map
 * the context's configuration (k, prefix, KMER_FLAG_CANONICAL or not, step 1)
 * builds from a file holding that record alone --
 *   not canonical: for every forward window w of the sequence, key w if w
 *                  starts with the prefix, and key rc w if rc w does;
 *   canonical:     the smaller string of {w, rc w}, if it starts with the prefix.
 * A window with a byte outside upper-case A/C/G/T gives no key (those are
 * record keys; the DB has none).  lengths[r] (kmer_db_template_stats) = the sum
 * of that Map's values over its A/C/G/T keys: one per (window, key) above, a
 * self-complementary window of a non-canonical configuration gives 2;
 * ulength[r] = the distinct such keys = the template's entries in the DB.
 *
 * `ctx` supplies k, the prefix, canonical or not, the device, the stream and
 * the scratch (its FASTA rewrite and line finder): any single-device context,
 * default ordered, KMER_FLAG_UNORDERED or KMER_FLAG_CANONICAL.  A chunk in
 * flight is settled first; the call may come before any session or after a
 * finish, and between stats, digest, lookup, screen, spectrum, extract, setops
 * and match calls: the context's finished results (host and device result,
 * table, bucket index, big list, extract buffers), kmer_lines, its records and
 * its session position are left unchanged.  The DB is independent of the
 * context (which may be reset or closed) and everything kmer_match_* does with
 * a DB works on it.
 * Checked before any device call -- KMER_E_BAD_PARAM: NULL ctx or out, NULL
 * bytes with len > 0, an unknown flag bit, k > 32, step != 1; KMER_E_STATE: a
 * group context, a session that has fed chunks and is not finished.
 * len == 0: KMER_OK and a DB of 0 templates.  A prefix with a byte outside
 * A/C/G/T, or longer than k: a valid DB whose templates all have ulength 0.
 * KMER_E_NONASCII as for a feed, KMER_E_OOM: the context stays usable.  2^32 - 1
 * or more window keys (before the dedup) or 2^31 - 1 or more templates:
 * KMER_E_BAD_PARAM with kmer_db_open's messages.  On any failure *out is NULL
 * and nothing is held.
 *
 * kmer_db_open_fasta_device: the bytes are in device memory, start at a record
 * start (offset 0 of a FASTA, or a '>' after '\n'), may end without '\n' and
 * may sit at any byte alignment; nothing outside [d_bytes, d_bytes + len) is
 * loaded.  The call waits for the work queued so far on `stream` (as the
 * lookup does); the DB is complete when it returns.
 * kmer_db_open_fasta: host bytes, uploaded in pieces cut before header lines
 * (the context's batch_bytes, default 64 MiB; a record longer than that is a
 * piece of its own): device and pinned memory are bounded by the piece plus
 * the (k-mer, template) pairs gathered so far; template indices run through
 * all pieces. */
enum { KMER_DB_PIECE_TEST = 1u };   /* debug: internal pieces of 4,096 windows, as KMER_SCREEN_PIECE_TEST */
kmer_status kmer_db_open_fasta_device(kmer_ctx *ctx, const void *d_bytes, size_t len, uint32_t flags,
                                      void *stream, kmer_db **out);
kmer_status kmer_db_open_fasta(kmer_ctx *ctx, const uint8_t *bytes, size_t len, uint32_t flags, kmer_db **out);
/* Per template, for templates [first, first + n) of any DB (either array may
 * be NULL): ulengths = its entries after the dedup; lengths = as defined above
 * for a FASTA DB, the number of keys the caller passed for it for a
 * kmer_db_open DB.  KMER_E_BAD_PARAM for a range past the DB's templates. */
kmer_status kmer_db_template_stats(kmer_db *db, uint32_t first, uint32_t n, uint64_t *lengths, uint64_t *ulengths);
/* The k-mers of template `tmpl` as ascending indices into the DB's distinct
 * k-mers (kmer_db_kmers decodes them), computed on the device from the
 * k-mer -> templates lists (no transpose is kept).  Up to `cap` entries;
 * *n = their number (the template's ulength). */
kmer_status kmer_db_template_kmers(kmer_db *db, uint32_t tmpl, uint64_t cap, uint32_t *idx, uint64_t *n);
/* The name of template `tmpl`: its header line without '>' and without the
 * trailing '\r' -- *len bytes at *name, owned by the DB (not terminated at
 * *len).  Length 0 for a headerless record and for a kmer_db_open DB. */
kmer_status kmer_db_template_name(const kmer_db *db, uint32_t tmpl, const char **name, uint32_t *len);
/* distinct = distinct k-mers, entries = (k-mer, template) pairs after dedup. */
kmer_status kmer_db_info(const kmer_db *db, uint32_t *k, uint32_t *n_templates, uint64_t *distinct,
                         uint64_t *entries);
/* Matches of the DB that are still open keep it alive: its device data is then
 * freed by the last kmer_match_close.  Do not pass `db` to any call afterwards
 * (offsets passed to kmer_match_open must start at 0 and not decrease:
 * KMER_E_BAD_PARAM otherwise). */
kmer_status kmer_db_close(kmer_db *db);

/* Round 1 (findKmersMatchesRedis): a query Map in iteration order — key i =
 * keys[offsets[i] .. offsets[i + 1]), counts[i] its value.  Scores every
 * template: uScore = query k-mers it holds, tScore = the sum of their counts;
 * hits = (k-mer, template) pairs.  The query is copied; the DB must outlive
 * the match. */
kmer_status kmer_match_open(kmer_db *db, const char *keys, const uint64_t *offsets, const uint64_t *counts,
                            uint64_t n, kmer_match **out);
/* The same from device memory (e.g. kmer_result_device of a count): n keys of
 * klen bytes back to back, uint64 counts.  `stream` (hipStream_t, NULL = the
 * legacy default stream): the match waits for the work queued on it so far. */
kmer_status kmer_match_open_device(kmer_db *db, const void *d_keys, uint32_t klen, const void *d_counts,
                                   uint64_t n, void *stream, kmer_match **out);
/* The same with a table-mode count as the query (KMER_FLAG_UNORDERED /
 * KMER_FLAG_CANONICAL, after a table finish): the Map that `ctx`'s finished
 * table describes — the one its host result lists and its lookup answers for.
 * The join runs from the DB's side, on the device, where the table lies:
 *   - query k-mer i is the DB's i-th distinct k-mer in ascending string order
 *     (A < C < G < T); n = the DB's distinct count (kmer_db_info);
 *   - a DB k-mer is in the query iff its Map value is > 0, and that value is
 *     its count.  The value is the lookup's: 0 unless the key starts with the
 *     context's prefix (canonical mode: and is the smaller string of the key
 *     and its reverse complement); a self-complementary key counts both
 *     strands' windows (not in canonical mode); keys with a byte outside
 *     A/C/G/T are never matched (the DB has none).
 * The table's host result is sorted by key bytes, as the DB's distinct k-mers
 * are, so templates, first-hit order, DB order, uScore, tScore, hits, every
 * winner and the scores after every remove equal those of the host-array open
 * over that host result in its own order.  Only a query index means something
 * else: an index into the DB's distinct k-mers (template_kmers; `removed`
 * writes `distinct` bytes); the DB decodes such indices back into k-mers.
 * The counts are copied: after the call the context may be reset, reused or
 * closed; its table is left unchanged.  A chunk still in flight on the
 * context is settled first.
 * KMER_E_STATE: a group context, a context not in table mode or without a
 * table finish.  KMER_E_BAD_PARAM: the context is on another device than the
 * DB.  A context whose k differs from the DB's gives a match without hits
 * (strings of different length never compare equal), as an empty table or an
 * empty DB does.  An exchanged table matches its own share of the classes. */
kmer_status kmer_match_open_table(kmer_db *db, kmer_ctx *ctx, kmer_match **out);
/* The DB's distinct k-mers [first, first + n) in ascending order, n * k bytes
 * back to back.  KMER_E_BAD_PARAM for a range past `distinct`. */
kmer_status kmer_db_kmers(const kmer_db *db, uint64_t first, uint64_t n, char *keys);
/* Current hits (sum of uScore) and templates with uScore > 0. */
kmer_status kmer_match_info(kmer_match *m, uint64_t *hits, uint32_t *n_templates);

enum { KMER_ORDER_FIRST_HIT = 0, KMER_ORDER_DB = 1 };
/* The templates with uScore > 0 and their current scores, in first-hit order
 * (the Redis path's templates Map) or DB order (the Mongo aggregation's).
 * Up to `cap` entries; *n = the number of such templates. */
kmer_status kmer_match_templates(kmer_match *m, uint32_t order, uint32_t cap, uint32_t *tmpl, uint64_t *uscore,
                                 uint64_t *tscore, uint32_t *n);

/* The round-1 query k-mers of template `tmpl` as query indices, ascending
 * (the `kmers` Set of its templates-Map entry, lib/kmerFinderServer.js:190-198).
 * Up to `cap` entries; *n = their number. */
kmer_status kmer_match_template_kmers(kmer_match *m, uint32_t tmpl, uint64_t cap, uint32_t *qidx, uint64_t *n);

typedef struct {
    uint32_t tmpl;          /* template index; UINT32_MAX when no template has hits */
    uint32_t reserved;
    uint64_t uscore, tscore; /* current scores of the winner */
    uint64_t hits;           /* current hits (results.hits of this round) */
    uint64_t first_uscore, first_tscore; /* its round-1 scores (kmerObject.firstMatches) */
} kmer_winner;
/* findWinner's pick: the largest uScore, ties to the earliest first hit. */
kmer_status kmer_match_winner(kmer_match *m, kmer_winner *w);
/* removeWinnerKmers(tmpl) + getMatches: every query k-mer of template `tmpl`
 * still in the query leaves it; all scores drop accordingly.  *hits = the
 * hits left. */
kmer_status kmer_match_remove(kmer_match *m, uint32_t tmpl, uint64_t *hits);
/* flags[i] = 1 iff query k-mer i was removed (n bytes). */
kmer_status kmer_match_removed(kmer_match *m, uint8_t *flags);
kmer_status kmer_match_close(kmer_match *m);

/* Message of the last failed kmer_db_* / kmer_match_* call on this thread. */
const char *kmer_match_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* KMER_MATCH_H */
