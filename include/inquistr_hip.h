/*
 * inquistr_hip.h — C ABI of the MI355X-native `inquiSTR call` hot path.
 *
 * What this boundary replaces in the reference (wdecoster/inquiSTR @ v0.13.0):
 * the reference has no FFI; the per-locus seam is
 *     genotype_repeat_phased(&mut IndexedReader, RepeatInterval, minlen, support)   src/call.rs:329-374
 *     genotype_repeat_unphased(...)                                                  src/call.rs:279-327
 * called once per locus from the serial loop (src/call.rs:150-157) or from a rayon
 * worker (src/call.rs:115-136).  A per-locus call cannot feed a GPU, so the ABI is
 * batch level: the host decodes BAM records (rust-htslib in the reference, the C++
 * front end in this repo), packs them into the buffers below and asks for the two
 * per-haplotype medians of every locus in one call.  Everything from "is this
 * record yielded by fetch()" (src/call.rs:288,338) through call_from_cigar
 * (src/call.rs:377-413) to median_str_length (src/call.rs:497-522) runs on the GPU.
 *
 * Plain C: pointers and sizes only, no C++/torch types.  Caller owns every buffer;
 * the library keeps no pointer after a call returns.
 */
#ifndef INQUISTR_HIP_H
#define INQUISTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define INQ_ABI_VERSION 5

/* ---- error codes (0 = ok, negative = failure; never throws / aborts) ---- */
enum {
    INQ_OK = 0,
    INQ_ERR_ARG = -1,          /* NULL pointer, inconsistent sizes, non-monotone CSR               */
    INQ_ERR_SUPPORT_ZERO = -2, /* support == 0: reference underflows `len/2 - 1` (src/call.rs:516) */
    INQ_ERR_PHASE = -3,        /* a read that passes the phased filter has HP > 2:
                                  reference `calls.get_mut(&phase).unwrap()` panics (src/call.rs:358) */
    INQ_ERR_CIGAR_OP = -4,     /* CIGAR op code > 8: rust-htslib's cigar() panics (src/call.rs:382)  */
    INQ_ERR_LOCUS = -5,        /* locus start < 10 (u32 underflow, src/call.rs:285,335) or end < start
                                  (src/repeats.rs:102-104)                                           */
    INQ_ERR_RANGE = -6,        /* pos + reference span of a read does not fit 31 bits (not a valid BAM) */
    INQ_ERR_INDEX = -7,        /* pair_read[] or a read's CIGAR extent points outside the buffers    */
    INQ_ERR_HIP = -8,          /* HIP runtime failure; see inq_last_error()                         */
    INQ_ERR_NOMEM = -9,
    INQ_ERR_NO_DEVICE = -10,   /* no gfx950 device visible: the library has NO CPU fallback          */
    INQ_ERR_INFLATE = -11,     /* device front end: a BGZF block does not inflate to its ISIZE (htslib: read error,
                                  `r.expect("Error reading BAM file")` src/call.rs:295,346 panics)     */
    INQ_ERR_BAM = -12,         /* device front end: record chain / field lengths corrupt, or records of the
                                  contig not coordinate-sorted                                          */
    INQ_ERR_AUX = -13          /* an aux field the reference panics on: HP of a FETCHED read is neither `C`
                                  nor `i` in phased mode (get_phase runs before the filter, src/call.rs:349,
                                  482-491; device front end), or a KEPT read carries INQ_READ_SA_PANIC
                                  (is_accidental_2d is only reached from call_from_cigar, i.e. for reads
                                  that passed the filter: src/call.rs:303,357 -> :394 -> :429-451)        */
};

/* ---- read descriptor: one 16-byte record per decoded BAM record ---------
 * Replaces rust-htslib bam::Record accessors used on the path:
 *   reference_start() src/call.rs:297,351,380   -> pos
 *   mapq()            src/call.rs:299,352       -> mapq
 *   cigar()           src/call.rs:382           -> cigar_off4 / n_cigar into inq_batch_t.cigar
 *   aux(b"HP")        src/call.rs:482-491       -> bits&INQ_READ_HAS_HP, phase (value `as u8`)
 *   is_accidental_2d  src/call.rs:415-459       -> bits&INQ_READ_IS_2D / INQ_READ_SA_PANIC (the SA string is evaluated
 *                                                  by whoever builds the descriptors: host sweep or cigar_gather)
 *   flag 0x4          (bam_endpos rule)         -> bits&INQ_READ_UNMAPPED
 */
typedef struct inq_read {
    uint32_t cigar_off4; /* first CIGAR word of this read, in units of 4 words (16 bytes)     */
    uint32_t n_cigar;    /* number of CIGAR ops                                               */
    int32_t pos;         /* BAM core.pos, 0-based leftmost                                    */
    uint8_t mapq;
    uint8_t bits;        /* INQ_READ_* */
    uint8_t phase;       /* HP value truncated to u8; meaningful iff INQ_READ_HAS_HP          */
    uint8_t promise;     /* INQ_READ_CHECKED or 0 (see below)                                 */
} inq_read_t;

/* promise: INQ_READ_CHECKED says that the producer of the descriptor has checked the domain rules of this read:
 * every op code is <= 8, pos >= -1 and pos + 1 + reference span < 2^31.  The device then reads the CIGAR of such a
 * read only as far as the locus window needs (up to the op after which pos + consumed >= end + 10) and does not
 * look for INQ_ERR_CIGAR_OP / INQ_ERR_RANGE in the rest, nor in the part it reads when every read offered beside it
 * is promised too.  A false promise may therefore leave the read's domain errors unreported; results for valid
 * reads are the same either way.  0 = no promise: every op is read and checked. */
#define INQ_READ_CHECKED 0x01u

#define INQ_READ_UNMAPPED 0x01u /* BAM flag 0x4   */
#define INQ_READ_REVERSE 0x02u  /* BAM flag 0x10  */
#define INQ_READ_HAS_HP 0x04u   /* HP aux present */
#define INQ_READ_IS_2D 0x08u    /* is_accidental_2d(record) == true */
#define INQ_READ_SA_PANIC 0x10u /* the CIGAR has an S op AND is_accidental_2d(record) would panic (SA aux not `Z`,
                                   no entry, < 4 fields, POS or CIGAR unparsable: src/call.rs:429-451,469).  The
                                   reference only gets there for a read that passed the filter (:303,357), so the
                                   device raises INQ_ERR_AUX iff such a read is KEPT; a filtered-out one is ignored */

/* ---- one batch of loci ----------------------------------------------------
 * cigar   : BAM-native packed ops, `len << 4 | op`, op in 0..8 = MIDNSHP=X, all reads
 *           concatenated.  Every read starts on a 4-word boundary; the 0..3 words of
 *           padding behind a read must be 0 (`0M`, a no-op for every rule on the path).
 *           n_cigar_words counts the padding and is a multiple of 4.
 * pairs   : CSR over loci.  pair_read[locus_pair_off[j] .. locus_pair_off[j+1]) are the
 *           reads offered to locus j IN FILE ORDER (the order rc_records() yields them,
 *           src/call.rs:294,345).  The list may be a superset of what fetch() would
 *           yield: the device applies htslib's overlap rule itself
 *           (pos < end_ext && bam_endpos > start_ext), so extra candidates change nothing.
 * loci    : un-extended BED coordinates (src/repeats.rs:75-79); the ±10 extension
 *           (src/call.rs:285-286,335-336) is applied on the device.
 */
typedef struct inq_batch {
    uint64_t n_reads;
    uint64_t n_cigar_words;
    uint64_t n_pairs;
    uint64_t n_loci;
    const uint32_t *cigar;          /* [n_cigar_words], 16-byte aligned */
    const inq_read_t *reads;        /* [n_reads]                        */
    const uint32_t *pair_read;      /* [n_pairs] index into reads       */
    const uint64_t *locus_pair_off; /* [n_loci + 1]                     */
    const uint32_t *locus_start;    /* [n_loci]                         */
    const uint32_t *locus_end;      /* [n_loci]                         */
    uint32_t minlen;                /* -m, src/main.rs:43               */
    uint32_t support;               /* -s, src/main.rs:47  (>= 1)       */
    uint32_t unphased;              /* -u, src/main.rs:55  (0 / 1)      */
    uint32_t reserved;              /* must be 0                        */
} inq_batch_t;

/* ---- results --------------------------------------------------------------
 * phase1/phase2 : Genotype.phase1/.phase2 (src/call.rs:27-31): exact integers or
 *                 halves, quiet NaN where the reference returns NAN (src/call.rs:499).
 * pair_call     : optional (may be NULL) per-pair Call value (src/call.rs:67-71)
 * pair_bits     : optional (may be NULL) per-pair INQ_PAIR_* bits
 * n_tie_loci    : unphased only: loci whose median split (src/call.rs:312-314) cuts
 *                 through equal values of mixed Span/Clip, where Rust's unstable sort
 *                 makes the reference itself ambiguous; this library orders ties by
 *                 file order (exact for <= 20 reads).
 */
typedef struct inq_result {
    double *phase1;     /* [n_loci] */
    double *phase2;     /* [n_loci] */
    int64_t *pair_call; /* [n_pairs] or NULL */
    uint8_t *pair_bits; /* [n_pairs] or NULL */
    uint64_t n_tie_loci;
} inq_result_t;

#define INQ_PAIR_CLIP 0x01u    /* Call::Clip (a soft clip was counted)            */
#define INQ_PAIR_FETCHED 0x02u /* yielded by fetch(): pos < end_ext && endpos > start_ext */
#define INQ_PAIR_KEPT 0x04u    /* survived the read filter (src/call.rs:297-302 / 349-355) */

/* Per-locus flags (the *_flags entry points below): one byte per locus, 0 or INQ_LOCUS_TIE.  INQ_LOCUS_TIE marks exactly the loci
 * counted in n_tie_loci (unphased only; a phased batch leaves every flag 0), so the flags of a batch sum to its n_tie_loci. */
#define INQ_LOCUS_TIE 0x01u

/* Per-locus read evidence (the *_evidence entry points below): what stands behind a row's two medians.  Counted on the device from
 * the per-pair outputs above, behind the locus kernels.  phase1 is NaN exactly when n_group1 < support, phase2 when n_group2 < support
 * (median_str_length, src/call.rs:498), and n_fetched >= n_kept >= n_group1 + n_group2 >= n_clip. */
typedef struct inq_locus_evidence {
    uint32_t n_fetched;  /* pairs with INQ_PAIR_FETCHED: what fetch() yields (src/call.rs:288,338)            */
    uint32_t n_kept;     /* pairs with INQ_PAIR_KEPT: passed the read filter (:297-302 / :349-355);
                            phased: reads with HP 0 included, which no group takes                          */
    uint32_t n_group1;   /* Calls behind phase1. phased: kept reads with HP 1. unphased: n_kept / 2 (:314)  */
    uint32_t n_group2;   /* Calls behind phase2. phased: kept reads with HP 2. unphased: n_kept - n_kept / 2 */
    uint32_t n_clip;     /* Calls of group 1 or 2 that are Call::Clip (INQ_PAIR_CLIP)                       */
    uint32_t reserved;   /* written as 0                                                                    */
    int64_t call_min;    /* smallest / largest Call value over groups 1 and 2; both 0 when                  */
    int64_t call_max;    /* n_group1 + n_group2 == 0                                                        */
} inq_locus_evidence_t;

/* The per-read Calls behind each row (the *_reads entry points below): one record per kept pair (INQ_PAIR_KEPT), compacted on the
 * device from the per-pair outputs above, behind the locus kernels (and the evidence launches).  Per batch two arrays: kept_off[n_loci + 1]
 * (u64, kept_off[0] = 0) and the records; locus j owns records [kept_off[j], kept_off[j + 1]), its kept pairs in file (pair) order,
 * so kept_off[j + 1] - kept_off[j] is the evidence record's n_kept.  The Calls median_str_length is handed (src/call.rs:312-314 / :358)
 * are, phased, the records of group 1 and of group 2; unphased, the records stable-sorted by value, the first len / 2 and the rest. */
#define INQ_READ_CALL_CLIP 0x01u
typedef struct inq_read_call {   /* 16 bytes, every byte written */
    int64_t  call;      /* the Call's value (pair_call) */
    uint32_t read;      /* index into the batch's reads[] (pair_read of the pair) */
    uint8_t  group;     /* phased: the read's HP (0, 1, 2); unphased: 0 */
    uint8_t  flags;     /* INQ_READ_CALL_CLIP = Call::Clip */
    uint16_t reserved;  /* 0 */
} inq_read_call_t;

/* Who a record of the per-read Calls is: the read's origin (position, strand, MAPQ) and, through name_len, its name (QNAME).  Produced by
 * the device front end only (inq_call_span_deferred_names / inq_call_flush_origins below): its records exist nowhere but in the inflated
 * bytes of a span slot, so the names are gathered on the device, at span time into the deferred batch and at flush time for the kept
 * records.  A caller of the host-buffer entries owns its batch and needs none of this: `read` indexes its own reads. */
typedef struct inq_read_origin {  /* 8 bytes, every byte written; one per record of inq_read_calls_fetch, same order */
    int32_t  pos;       /* inq_read_t.pos */
    uint8_t  mapq;
    uint8_t  bits;      /* INQ_READ_* of the descriptor (REVERSE is what the table prints) */
    uint16_t name_len;  /* 0 .. 254: bytes of the name, no terminator */
} inq_read_origin_t;

/* The bases behind a Call: which part of the read's SEQ lies over the locus window.  Per (locus, read) pair take the window the locus
 * kernels build, se = start - 10 and ee = end + 10 (both u32), and walk the read's CIGAR as the batch holds it (a long CIGAR from
 * CG:B,I already swapped in).  The reference cursor r starts at pos, the query cursor at 0; arithmetic is 64-bit and never wraps.
 * For a reference coordinate x,
 *     Q(x) =  sum over I and S ops       len * [r_op < x]
 *           + sum over M, = and X ops    clamp(x - r_op, 0, len)
 * with r_op the reference cursor in front of the op; D and N move r only, H, P and op codes above 8 move nothing.  Then
 *     q_beg = min(Q(se), l_seq),  q_end = min(Q(ee - 1), l_seq),  n_bases = q_end - q_beg,
 * and the slice is SEQ bases [q_beg, q_end).  A window with ee - 1 <= se as integers - those of width 0, empty or wrapped, start < 9
 * among them, and start = 9, whose se is 2^32 - 1 (no entry that calls accepts a start below 10) -, or a read index or descriptor
 * outside the batch, gives (0, 0); l_seq == 0 (SEQ `*`) gives n_bases 0; a CIGAR whose query length disagrees with l_seq
 * is only ever cut, never read past.
 * An I or S op is in the slice exactly when se <= r_op <= ee - 2, which is exactly when call_from_cigar (src/call.rs:388-401,
 * start < reference_position < end) would count it, whatever minlen; the M bases are those at reference coordinates [se, ee - 1).
 * So n_bases = matched bases in the window + inserted + clipped bases in the window; a read that starts inside the window has
 * q_beg = 0, its leading soft clip included, and one that ends inside it runs to l_seq.
 * Bases stay as the BAM stores them: reference-forward, 4-bit codes (`=ACMGRSVTWYHKDBN`).  A slice is packed two bases to a byte,
 * re-aligned so that its first base is the high nibble of its first byte; a last odd low nibble is 0: (n_bases + 1) / 2 bytes. */
typedef struct inq_read_seq {  /* 8 bytes, every byte written; one per record of inq_read_calls_fetch, same order */
    uint32_t q_beg;    /* 0-based offset into SEQ as stored */
    uint32_t n_bases;
} inq_read_seq_t;

/* How much of those bases is the locus's motif: the pure runs of the motif in a kept record's slice.
 * Motif word, one uint64_t per locus: nibble 15 is k, the motif length, 1 .. 15; nibbles 0 .. k - 1 are the motif's bases m[0 .. k) as
 * BAM codes (A = 1, C = 2, G = 4, T = 8); the nibbles between are not read.  A word is "no motif" when k = 0 or when any of nibbles
 * 0 .. k - 1 is not one of those four codes.  The device checks this itself: no word makes it read or write out of bounds.
 * Let s[0 .. n) be the slice of a kept record: the n_bases 4-bit codes inq_read_seq_t describes, indexed from the slice's first base.
 * For a rotation r in [0, k), position i HITS when s[i] == m[(i + r) mod k]; equality is exact, so `=`, N and every ambiguity code
 * hit nothing.  A RUN is a maximal interval [a, b) of consecutive hits at one rotation, and R is the set of all runs of all k
 * rotations.  Then
 *     run_beg, run_len   the longest run in R (a, b - a); on a tie the one with the smallest a; (0, 0) when R is empty.  A run
 *                        shorter than k counts here
 *     motif_bases        the number of positions that lie in at least one run of R with b - a >= k
 *     n_runs             the number of runs in R with b - a >= k
 * No motif, or n = 0, gives four zeros.  The word is taken literally: a non-primitive one (CAGCAG) has identical runs at equivalent
 * rotations and each counts in n_runs.  The host encoder, inq_host_motif_encode of include/inquistr_host.h, reduces a motif to its
 * primitive root; for a
 * primitive motif no run of length >= k at one rotation is a run at another or contains one, so n_runs is the number of distinct
 * maximal pure stretches and n_runs - 1 the number of interruptions and phase shifts.  Runs of different rotations may overlap by up
 * to k - 1 bases (a one-base deletion inside the repeat); motif_bases is the union. */
typedef struct inq_read_motif {  /* 16 bytes, every byte written; one per record of inq_read_calls_fetch, same order */
    uint32_t run_beg;      /* 0-based offset into the slice */
    uint32_t run_len;
    uint32_t motif_bases;
    uint32_t n_runs;
} inq_read_motif_t;

/* Which short motif a locus's kept reads repeat, for a caller who has no catalogue motif or wants the catalogue's checked against the
 * reads.  Take locus j with kept records kept_off[j] .. kept_off[j + 1], all groups (h1 / h2 / other); each record's slice is s[0 .. n),
 * the codes inq_read_seq_t describes; a code is a BASE when it is one of 1, 2, 4, 8.  All of it is integer arithmetic and independent
 * of the records' order:
 *     lag counts   for k = 1 .. 6, T_k = the sum over the records of the number of i with k <= i < n, s[i] == s[i - k], s[i] a base
 *     period       p = the smallest k with T_k == max_j T_j when that maximum is above 0; else p = 0 and the record is all zeros
 *                  except `bases`
 *     copies       for each record and each i with i + 2 p <= n: if s[i .. i + p) are all bases and s[i + t] == s[i + p + t] for every
 *                  t < p, the p-mer s[i .. i + p) gets one count
 *     class        a p-mer's class is its lexicographically smallest rotation under A < C < G < T, a class's count the sum over its
 *                  members; the class with the largest count wins, among equal counts the lexicographically smallest.  No count at
 *                  all: word = 0, copies = 0, period = p still
 *     word         the winner reduced to its primitive root (ACAC at p = 4 becomes AC; the root of a smallest rotation is itself a
 *                  smallest rotation), as the motif word of inq_read_motif_t: k in nibble 15, BAM codes in nibbles 0 .. k - 1.  So
 *                  CAG repeats give AGC, and the word is never a non-primitive one.
 * Motifs longer than 6 bases are not looked for: they stay the catalogue's business.  Known limit: a locus with little repeat in its
 * reads is often given a shorter period than its motif's - two or three copies of a 5- or 6-mer between random flanks have fewer lag-p
 * hits than the chance hits at lags 1 .. 3 of the flanks (measured: DESIGN.md, "Locus motifs"). */
typedef struct inq_locus_motif {   /* 40 bytes, every byte written; one per locus */
    uint64_t word;     /* motif word, 0 = none found */
    uint64_t period;   /* p, 0 .. 6 */
    uint64_t bases;    /* sum of n over the locus's kept records, every code counted */
    uint64_t tandem;   /* T_p */
    uint64_t copies;   /* the winning class's count */
} inq_locus_motif_t;

typedef struct inq_ctx inq_ctx_t;

/* Opens HIP device `device_id` (must be gfx950), creates the library's stream and
 * scratch.  One ctx per device; a ctx serves one caller at a time. */
int inq_ctx_create(int device_id, inq_ctx_t **out);
/* The same in a hurry: *ctx is set and *stage_ready raised (release store) as soon as inq_span_stage / _begin / _wait may be called
 * on it from another thread, ~30 ms before the function returns; every other entry point only after it has returned INQ_OK.  A
 * context that was published stays valid until inq_ctx_destroy, whatever the return value (the caller destroys it). */
int inq_ctx_create_early(int device_id, inq_ctx_t **ctx, volatile int *stage_ready);
/* The list form ("inq_ctx_create(device_ids, n, &ctx)"; the reference's counterpart is rayon's pool of workers,
 * src/call.rs:104-118): one context per entry of device_ids - an ordinal may repeat -, made concurrently (each on a thread of
 * its own: the runtime's start-up is paid once, the per-device parts side by side); ctxs[0 .. n) receive them.  All or nothing: on
 * failure every context that was made is destroyed again, ctxs[] is all NULL and the first failing entry's code is returned.  Each
 * context is then driven by its own host thread (a ctx serves one caller at a time; distinct ctxs are independent). */
int inq_ctx_create_multi(const int *device_ids, int n, inq_ctx_t **ctxs);
void inq_ctx_destroy(inq_ctx_t *ctx);

/* Host-buffer entry: batch and result point to HOST memory (pinned for best H2D).
 * Validates the batch, uploads, runs the kernels, downloads, synchronises. */
int inq_call_batch(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result);

/* Device-resident entry: every pointer in batch/result is a DEVICE pointer on the
 * ctx's device; hip_stream is a hipStream_t (NULL = the ctx's own stream).  Enqueues
 * only — no host synchronisation, no allocation.  result->n_tie_loci is not written;
 * fetch it, and any domain error the kernels flagged, with inq_ctx_status() after
 * the stream has been synchronised. */
int inq_call_batch_device(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result,
                          void *hip_stream);
/* The two entries above with per-locus flags (INQ_LOCUS_TIE): locus_flags[j] belongs to locus j of the batch; HOST memory of
 * n_loci bytes for inq_call_batch_flags, DEVICE memory on the ctx's device (enqueued like the rest) for the device form.  NULL = no
 * flags: exactly inq_call_batch / inq_call_batch_device.  The array is zeroed on the launch stream in front of the kernels. */
int inq_call_batch_flags(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result, uint8_t *locus_flags);
int inq_call_batch_device_flags(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result, uint8_t *d_locus_flags,
                                void *hip_stream);

/* ... and with per-locus evidence: evidence[j] belongs to locus j of the batch; HOST memory of n_loci records for
 * inq_call_batch_evidence (locus_flags may be NULL; per-pair outputs the caller did not ask for are kept in context scratch), DEVICE
 * memory for the device form, which allocates nothing and therefore needs result->pair_call and result->pair_bits when d_evidence is
 * given (INQ_ERR_ARG otherwise).  NULL = no evidence: exactly the *_flags entries, nothing more is enqueued or allocated.  Two launches
 * behind the locus kernels write every byte of every record.  A batch that ends in a domain error leaves the evidence unspecified. */
int inq_call_batch_evidence(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result, uint8_t *locus_flags,
                            inq_locus_evidence_t *evidence);
int inq_call_batch_device_evidence(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result, uint8_t *d_locus_flags,
                                   inq_locus_evidence_t *d_evidence, void *hip_stream);

/* ... and with the per-read Calls (inq_read_call_t above); locus_flags and evidence may be NULL.
 * Device form: d_kept_off = DEVICE [n_loci + 1] u64, d_kept = DEVICE [n_pairs] records, 16-byte aligned; allocates no output and only
 * enqueues: three launches (count per tile of inq_read_call_tile() pairs, scan of the tiles, scatter) behind the locus kernels and the
 * evidence launches write every byte of d_kept_off and of the records [0, d_kept_off[n_loci]); records at and behind that are not
 * written.  Like the evidence form it needs result->pair_call and result->pair_bits (INQ_ERR_ARG otherwise, nothing enqueued); one of
 * the two pointers without the other is INQ_ERR_ARG; both NULL = exactly inq_call_batch_device_evidence.
 * Host form: kept_off = HOST [n_loci + 1], brought down with the rows; per-pair outputs the caller did not ask for and the records
 * stay in context scratch, the records until the context's next call: inq_read_calls_fetch copies the first n of them (n above the last
 * call's total, kept_off[n_loci]: INQ_ERR_ARG; a call without the lists has a total of 0).  kept_off NULL = exactly
 * inq_call_batch_evidence.  A batch that ends in a domain error leaves the lists unspecified. */
int inq_call_batch_reads(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result, uint8_t *locus_flags,
                         inq_locus_evidence_t *evidence, uint64_t *kept_off);
int inq_call_batch_device_reads(inq_ctx_t *ctx, const inq_batch_t *batch, inq_result_t *result, uint8_t *d_locus_flags,
                                inq_locus_evidence_t *d_evidence, uint64_t *d_kept_off, inq_read_call_t *d_kept, void *hip_stream);
int inq_read_calls_fetch(inq_ctx_t *ctx, inq_read_call_t *out, uint64_t n);
/* pairs per workgroup of the compaction (a constant of the build) */
uint32_t inq_read_call_tile(void);

/* Device-side status of the launches since the last inq_ctx_status() call: returns
 * INQ_OK or the first domain error (INQ_ERR_PHASE / _CIGAR_OP / _LOCUS / _RANGE /
 * _INDEX) and the tie count.  Synchronises the device. */
int inq_ctx_status(inq_ctx_t *ctx, uint64_t *n_tie_loci);

/* Kernel timing with HIP events on the launch stream (for bench.py's roofline block).
 * which: 0 = whole inq_call_batch_device launch sequence, 1 = the CIGAR-walk kernel,
 * 2 = the BGZF inflate kernel of the last inq_bgzf_inflate / inq_call_span (launches = 1).
 * Returns accumulated milliseconds and launch count since the last reset.  A sequence that is the CIGAR-walk kernel alone (a depth
 * hint of at most 64 reads; no evidence, per-read Calls or other side output that a kernel behind it writes) is timed by the two
 * events around that kernel: which = 0 and which = 1 then return the same time. */
int inq_ctx_timing_enable(inq_ctx_t *ctx, int on);
int inq_ctx_timing_read(inq_ctx_t *ctx, int which, double *total_ms, uint64_t *launches);
int inq_ctx_timing_reset(inq_ctx_t *ctx);

/* Tuning knobs.  key: "grid_medium" = workgroups of the kernel that takes the 65..256-read loci and walks the deeper ones
 * (default 4096); "grid_tail" ("grid_big" up to ABI v4) = workgroups of the persistent kernel that reduces the deeper ones (default
 * 256, never more than the device's compute units: they meet at grid barriers); "grid_side" = 1 .. 65535: no launch of a side
 * kernel (the locus and read motif kernels, the window walk, the packed gather, the byte gather of names and slices, the origins, the
 * slices' records) has more workgroups than that - each takes every gridDim.x-th tile, so the outputs do not change; 0 (default) =
 * each launch's own cap (65 536 workgroups, 2^20 for the names and origins); anything else: INQ_ERR_ARG; "max_reads_hint" = N > 0 promises that no locus of
 * the following batches is offered more than N reads (N <= 64 skips the two launches behind the first kernel - which cost a few
 * microseconds when nothing deep is there; a violated promise is reported as INQ_ERR_ARG), 0 (default) = unknown;
 * "verify_crc" = 0 skips the CRC32 check of the device front end (default 1);
 * "inflate_algo" = 0 or 2: accepted, no effect - the inflate runs one workgroup per BGZF block, the one kernel there is (0 named
 * it and 2 meant "the quicker one" while a lane-per-block kernel was selectable as 1); 1 and any other value: INQ_ERR_ARG;
 * "inflate_lit_pairs" = 1 / 0: the workgroup inflate's symbol loop decodes a second literal from the same 32 bits as the first
 * (+18 - 24 % on sequence / quality bytes) or not (CIGAR-only records lose 4.6 % to the wasted look); -1 (default) = decided per
 * call from the code lengths in a few sampled block headers;
 * "inflate_tokens" = 1: the workgroup inflate keeps the symbols its counting passes decode (32 KB of device scratch per BGZF
 * block) so that its commit step does not decode them again (+3 - 4 % on match-heavy blocks, -2 ... -5 % on sequence / quality
 * bytes, and four times the HBM traffic of the inflate: the stores cost what the second decode did), 0 (default since round 4) =
 * it decodes again, -1 = on for spans whose sampled block headers say match-heavy (round 3's default);
 * "blocking_sync" = 1: every wait of this context gives its core back (hipDeviceScheduleBlockingSync; as a process default - set
 *   before the context is made - also a blocking upload event) instead of spinning.  Default 0: spinning costs two cores (the caller's
 *   thread during a span's inflate, the uploader's during its copy) and answers a few microseconds sooner; libinquistr_host.so sets 1
 *   by itself when a caller's share of the granted cores is below 8 (eight ranks on a 16-core grant), where those two cores are the
 *   readers'.
 * "inflate_ahead" = 1 (default since round 4): inq_span_stage inflates a span right behind its upload, on a stream of its own, so
 * that the inflate of span k + 1 runs next to span k's record scan, gather and join (costs one inflated buffer per staging slot:
 * device allocations cost microseconds, tools/alloc_probe.hip); 0 = the span is inflated when it is called;
 * "gather_nt" = 1 (default) / 0: the device front end's CIGAR gather stores with the non-temporal policy (the batch it builds is
 * read by a later launch); "batch_loci_hint" = N: inq_call_span_deferred sizes the batch's buffers for N loci from its first span;
 * "retired_limit_mb" / "test_fail_allocs": see inq_ctx_alloc_retries;
 * "nt_loads" = 1 / 0 forces the non-temporal cache policy for the CIGAR stream on / off; -1 (default)
 * picks it when no read is shared between loci (n_pairs <= n_reads). */
int inq_ctx_set_option(inq_ctx_t *ctx, const char *key, int64_t value);
/* How often a device allocation of this context met "out of memory", gave the buffers it had outgrown and parked back (options
 * "retired_limit_mb": how many MB may be parked, default 16384) and tried again - and, for the deferred batch's speculative
 * reserve, fell back to the bytes really needed.  ("test_fail_allocs" = N makes the next N first attempts fail: the test seam.) */
uint64_t inq_ctx_alloc_retries(const inq_ctx_t *ctx);
/* The same for every context made FROM NOW ON in this process (any thread): key and value are checked at once, the option is applied
 * inside inq_ctx_create / _early / _multi before the context is handed out.  For a host that does not make the contexts itself
 * (libinquistr_host.so does: `inquistr call --ctx-option key=value`).  The library reads NO option from the environment. */
int inq_default_option(const char *key, int64_t value);
/* INQ_OK and *value if the process default of `key` has been set (by inq_default_option), INQ_ERR_ARG otherwise: lets a host library
 * choose a default of its own ("blocking_sync" when its share of the cores is small) without overriding what its user asked for. */
int inq_default_option_get(const char *key, int64_t *value);

/* Page-locks caller-owned host memory in place (hipHostRegister: 0.5 ms for 268 MB of huge-page-backed memory, against 50 - 60 ms
 * for inq_alloc_pinned of the same size), so that copies from it are plain DMA.  The runtime must be up (a ctx exists). */
int inq_pin_host(void *p, size_t bytes);
void inq_unpin_host(void *p);

/* Pinned host allocations for batch buffers. */
int inq_alloc_pinned(size_t bytes, void **out);
void inq_free_pinned(void *p);


/* ==== device front end: BGZF inflate + BAM record scan + overlap join on the GPU =====================
 * Replaces, for one span of the file, what `bam.fetch((tid, start_ext, end_ext))` + `rc_records()` and the
 * record accessors do per locus in the reference (src/call.rs:288,294,297-299,338,345,351-352; [3P]
 * htslib bgzf.c / sam.c / hts.c): the host only reads the compressed bytes and walks the 18-byte BGZF
 * headers and the .bai; inflating, finding the records, decoding their fixed fields and HP / SA / CG
 * tags, and matching reads to loci with htslib's overlap rule all happen on the device, and the batch
 * the locus kernels consume never exists in host memory.
 */
typedef struct inq_bgzf_block {
    uint64_t comp_off; /* offset of the block's DEFLATE payload (behind its gzip header) in `comp`    */
    uint32_t comp_len; /* payload bytes, without the 8-byte CRC32 / ISIZE trailer                      */
    uint32_t isize;    /* inflated size from the trailer (<= 65536)                                    */
    uint64_t out_off;  /* where the block's data goes in the inflated byte string                      */
} inq_bgzf_block_t;

/* per-block inflate status bits (0 = the block inflated to exactly isize bytes) */
#define INQ_INFLATE_BAD_HEADER 0x01u    /* reserved block type, bad code-length set, extents outside the buffers */
#define INQ_INFLATE_BAD_CODE 0x02u      /* a bit pattern that is no code of the current Huffman set            */
#define INQ_INFLATE_INPUT_OVERRUN 0x04u /* the stream needs more bits than the payload holds                   */
#define INQ_INFLATE_OUTPUT_SIZE 0x08u   /* more or fewer bytes than isize                                      */
#define INQ_INFLATE_BAD_DISTANCE 0x10u  /* a match reaches in front of the block                               */
#define INQ_INFLATE_BAD_STORED 0x20u    /* stored block LEN / NLEN mismatch                                    */
#define INQ_INFLATE_BAD_CRC 0x40u       /* inflated bytes do not match the CRC32 of the block's trailer        */

/* Inflates n_blocks BGZF payloads; every pointer is HOST memory (the call uploads, runs one workgroup
 * per block - ctx option "inflate_algo" no longer selects anything: 0 and 2 are accepted, 1 is INQ_ERR_ARG -, downloads, synchronises).  block_status may be NULL.  Returns INQ_ERR_INFLATE if any block
 * failed.  `comp` holds whole BGZF blocks: the 8 bytes behind every payload are its CRC32 / ISIZE trailer,
 * and the inflated bytes are checked against that CRC32 as htslib does (ctx option "verify_crc", default 1). */
int inq_bgzf_inflate(inq_ctx_t *ctx, const uint8_t *comp, uint64_t comp_bytes, const inq_bgzf_block_t *blocks,
                     uint64_t n_blocks, uint8_t *out, uint64_t out_bytes, uint32_t *block_status);

/* One span: whole BGZF blocks of a coordinate-sorted BAM, as one or more SEGMENTS (runs of consecutive
 * blocks, ascending and disjoint in the file), plus loci whose overlapping records all start inside those
 * segments.  Segments let one call serve loci that are far apart without inflating what lies between. */
#define INQ_ANCHOR_SEGMENT_END (1ull << 63)
typedef struct inq_span {
    const uint8_t *comp;             /* HOST (pageable is fine): the compressed bytes of the blocks,
                                        segment after segment, each payload followed by its trailer      */
    uint64_t comp_bytes;
    const inq_bgzf_block_t *blocks;  /* file order; out_off dense and ascending from 0                   */
    uint64_t n_blocks;
    const uint64_t *anchors;         /* ascending offsets into the inflated bytes at which a BAM record
                                        is known to start (virtual offsets of the .bai: chunk begins and
                                        linear-index entries); every segment opens with one.  Records
                                        are found by following block_size from each anchor, one lane per
                                        anchor.                                                           */
    const uint64_t *anchor_stop;     /* [n_anchors] where chain i ends: the next anchor (the chain must
                                        land on it), or `end of the segment | INQ_ANCHOR_SEGMENT_END`
                                        (a record cut by the segment's end is dropped)                    */
    uint64_t n_anchors;
    const int32_t *locus_tid;        /* [n_loci] header().tid(chrom), src/call.rs:287,337                 */
    const uint32_t *locus_start;     /* [n_loci] un-extended BED coordinates, any order                   */
    const uint32_t *locus_end;
    uint64_t n_loci;
    uint32_t minlen, support, unphased, reserved;
} inq_span_t;

typedef struct inq_span_stats {
    uint64_t n_records;      /* records found in the span                                   */
    uint64_t n_reads;        /* of which placed on a contig (unplaced records close the file) */
    uint64_t n_pairs;        /* (locus, read) pairs = records fetch() would yield, summed    */
    uint64_t n_cigar_words;  /* gathered CIGAR words incl. padding                           */
    uint64_t inflated_bytes;
    uint32_t max_reads;      /* deepest locus                                                */
    uint32_t front_status;   /* raw status bits of the scan kernels (diagnostics)            */
    uint64_t first_bad_record;
    double ms_upload, ms_inflate, ms_scan, ms_join, ms_call; /* HIP-event times of the stages */
} inq_span_stats_t;

/* Runs the whole path for one span; result->phase1/phase2 (HOST, [n_loci]) receive the rows in the order
 * of locus_start/locus_end; pair_call / pair_bits are not produced (pass NULL).  stats may be NULL. */
int inq_call_span(inq_ctx_t *ctx, const inq_span_t *span, inq_result_t *result, inq_span_stats_t *stats);

/* Two-step form for files of many spans: inq_span_stage uploads the compressed bytes, the block table and the
 * anchors of a span into one of INQ_SPAN_SLOTS device-side slots (0 .. 7) on the library's copy stream and returns when they are
 * there; inq_call_span_staged then runs the span from that slot without uploading.  inq_span_stage may be
 * called from another host thread while an inq_call_span / inq_call_span_staged of an EARLIER span is in
 * progress on the same ctx (different slot): the upload of span k+1 then overlaps the inflate of span k.
 * A slot may be staged again once the call that used it has returned.  span->comp must be the same pointer
 * and sizes in both calls. */
#define INQ_SPAN_SLOTS 8 /* two sets of four: a session stages the next file's spans while this file's are called */
int inq_span_stage(inq_ctx_t *ctx, const inq_span_t *span, int slot);
/* The same in two steps, so that the copy engine goes from one span's bytes straight to the next one's: _begin enqueues the
 * upload (and the inflate behind it) and returns - the block table and the anchors are copied on the spot, span->comp must stay
 * until _wait(slot) has returned; a second span may be begun (other slot) before the first is waited for.  inq_span_stage =
 * _begin + _wait. */
int inq_span_stage_begin(inq_ctx_t *ctx, const inq_span_t *span, int slot);
int inq_span_stage_wait(inq_ctx_t *ctx, int slot);
int inq_call_span_staged(inq_ctx_t *ctx, const inq_span_t *span, int slot, inq_result_t *result,
                         inq_span_stats_t *stats);

/* Deferred form, for spans that hold too few loci to fill the chip on their own (a span of 256 MB of SEQ / QUAL-bearing records
 * holds under a thousand loci; the locus kernels want tens of thousands per launch): inq_call_span_deferred does everything
 * inq_call_span / inq_call_span_staged (slot >= 0) does up to the overlap join and APPENDS the span's batch - CIGARs, read
 * descriptors, pairs, loci - to a batch that stays on the device; inq_call_flush runs the locus kernels once over everything
 * appended since the last flush and returns the rows in the order the loci were appended (n_loci must be their number;
 * ms_call, if not NULL, receives the HIP-event time of the launch sequence).  minlen / support / unphased must be the same in
 * every span of one batch.  The reference's counterpart is still the per-locus loop of src/call.rs:115-136,150-157: which loci
 * share a launch is not observable in the rows. */
int inq_call_span_deferred(inq_ctx_t *ctx, const inq_span_t *span, int slot /* -1: not staged */, inq_span_stats_t *stats);
int inq_call_flush(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call);
/* inq_call_flush with the rows left ON THE DEVICE: row j of the flush goes to d_phase1[index[j]], d_phase2[index[j]] (DEVICE arrays of
 * `cap` entries on the ctx's device; index: HOST, n_loci entries, every one < cap), only the tie count and the status come back.  For a
 * caller whose rows travel on from device memory - one process per GPU: the RCCL gather of the per-shard rows to rank 0 (north_star;
 * inquistr_amd/call_dist.py) reads them where the kernels' rows already are. */
int inq_call_flush_device(inq_ctx_t *ctx, double *d_phase1, double *d_phase2, uint64_t cap, const uint32_t *index, uint64_t n_loci,
                          uint64_t *n_tie_loci, double *ms_call);
/* The two flushes above with per-locus flags (INQ_LOCUS_TIE): locus_flags = HOST [n_loci], entry j for the j-th locus of the
 * flush (append order), brought down with the rows; NULL = no flags. */
int inq_call_flush_flags(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags);
int inq_call_flush_device_flags(inq_ctx_t *ctx, double *d_phase1, double *d_phase2, uint64_t cap, const uint32_t *index, uint64_t n_loci,
                                uint64_t *n_tie_loci, double *ms_call, uint8_t *locus_flags);
/* inq_call_flush_flags with per-locus evidence: evidence = HOST [n_loci], record j for the j-th locus of the flush (append order);
 * NULL = exactly inq_call_flush_flags.  The per-pair arrays the counting needs live in context scratch sized from the batch's pairs. */
int inq_call_flush_evidence(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags,
                            inq_locus_evidence_t *evidence);
/* ... and with the per-read Calls: kept_off = HOST [n_loci + 1] in append order, NULL = exactly inq_call_flush_evidence; the records
 * through inq_read_calls_fetch, their `read` indexing the deferred batch's reads as inq_span_fetch_batch returns them. */
int inq_call_flush_reads(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags,
                         inq_locus_evidence_t *evidence, uint64_t *kept_off);
/* The names (QNAME) and origins of the reads behind those records.  A read's name is bytes [0, max(l_read_name, 1) - 1) of the record's
 * name field, as they stand (a NUL inside is the reader's to cut at; for l_read_name == 0 no name byte is read).
 * inq_call_span_deferred_names is inq_call_span_deferred that also gathers the names of the span's placed records into the deferred
 * batch (one scan of the lengths and one copy launch behind the CIGAR gather).  All spans of one batch with names or all without:
 * mixing is INQ_ERR_ARG at the offending append, which appends nothing.  inq_call_span / inq_call_span_staged produce no per-pair outputs
 * and take no names.
 * inq_call_flush_origins is inq_call_flush_reads plus, behind the compaction, one inq_read_origin_t per kept record and the kept
 * records' names back to back in record order; *name_bytes receives their total.  kept_off NULL or name_bytes NULL, or a batch
 * appended without names, is INQ_ERR_ARG (the batch stays).  Both stay in context scratch until the context's next call:
 * inq_read_origins_fetch copies the first n origins and the first name_bytes bytes of the names (the name of record k begins at the
 * sum of name_len of the records in front of it); n or name_bytes above the last flush's totals is INQ_ERR_ARG, and a flush without
 * origins has totals of 0.
 * inq_span_fetch_names (test / debug, beside inq_span_fetch_batch): the names of ALL reads of the batch the last flush ran on,
 * name_off[n_reads + 1] and the bytes (cap_bytes below the total, or a batch without names: INQ_ERR_ARG). */
int inq_call_span_deferred_names(inq_ctx_t *ctx, const inq_span_t *span, int slot, inq_span_stats_t *stats);
int inq_call_flush_origins(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags,
                           inq_locus_evidence_t *evidence, uint64_t *kept_off, uint64_t *name_bytes);
int inq_read_origins_fetch(inq_ctx_t *ctx, inq_read_origin_t *origins, uint64_t n, uint8_t *names, uint64_t name_bytes);
int inq_span_fetch_names(inq_ctx_t *ctx, uint64_t *name_off /* [n_reads + 1] */, uint8_t *names, uint64_t cap_bytes);
/* segments (names) per workgroup of the byte gather (a constant of the build) */
uint32_t inq_read_name_tile(void);
/* The bases behind those records (inq_read_seq_t above).
 * inq_call_span_deferred_seqs is inq_call_span_deferred_names that also cuts, for every pair of the span, the slice of the read's SEQ
 * over the locus window, out of the slot's inflated bytes into the deferred batch (the window walk behind the join, a scan of the
 * byte lengths whose total comes down with the append's last readback, the packed gather and one further stream wait).  All spans of
 * one batch with sequences or all without: mixing is INQ_ERR_ARG at the offending append, which appends nothing.
 * inq_call_flush_seqs is inq_call_flush_origins plus one inq_read_seq_t per kept record and the kept records' packed slices back to
 * back in record order, record k's (n_bases + 1) / 2 bytes beginning at the sum of those in front of it; *seq_bytes receives their
 * total.  seq_bytes NULL = exactly inq_call_flush_origins; with it, a batch appended without sequences is INQ_ERR_ARG (the batch
 * stays).  Both stay in context scratch until the context's next call: inq_read_seqs_fetch copies the first n records and the first
 * seq_bytes packed bytes; n or seq_bytes above the last flush's totals is INQ_ERR_ARG, and a flush without sequences has totals of 0.
 * inq_span_fetch_seqs (test / debug, beside inq_span_fetch_names): q_beg, n_bases, seq_off[n_pairs + 1] and the packed bytes of ALL
 * pairs of the batch the last flush ran on (each array may be NULL; cap_bytes below the total, or a batch without sequences:
 * INQ_ERR_ARG).
 * inq_seq_windows: the window walk alone over a host-buffer batch (uploaded like inq_call_batch's; minlen, support and unphased are
 * not read): q_beg[n_pairs] and n_bases[n_pairs].  l_seq[n_reads] cuts both as the contract says, NULL = no cut but at 2^32 - 1, what the results hold.  The result does not
 * depend on inq_read_t.promise. */
int inq_call_span_deferred_seqs(inq_ctx_t *ctx, const inq_span_t *span, int slot, inq_span_stats_t *stats);
int inq_call_flush_seqs(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags,
                        inq_locus_evidence_t *evidence, uint64_t *kept_off, uint64_t *name_bytes, uint64_t *seq_bytes);
int inq_read_seqs_fetch(inq_ctx_t *ctx, inq_read_seq_t *seqs, uint64_t n, uint8_t *packed, uint64_t seq_bytes);
int inq_span_fetch_seqs(inq_ctx_t *ctx, uint32_t *q_beg, uint32_t *n_bases, uint64_t *seq_off /* [n_pairs + 1] */, uint8_t *packed,
                        uint64_t cap_bytes);
int inq_seq_windows(inq_ctx_t *ctx, const inq_batch_t *batch, const uint32_t *l_seq /* [n_reads] */, uint32_t *q_beg,
                    uint32_t *n_bases /* [n_pairs] */);
/* pairs per workgroup and turn of the window walk (a constant of the build) */
uint32_t inq_seq_window_tile(void);
/* The motif runs of those bases (inq_read_motif_t above), computed on the device at flush time out of the batch's own slices.
 * inq_call_flush_motifs is inq_call_flush_seqs plus `motif`, a HOST array of one motif word per locus in append order, and one
 * inq_read_motif_t per kept record.  motif NULL = exactly inq_call_flush_seqs; with it, seq_bytes NULL or a batch appended without
 * sequences is INQ_ERR_ARG (the batch stays).  The records stay in context scratch until the context's next call:
 * inq_read_motifs_fetch copies the first n; n above the last flush's total is INQ_ERR_ARG, and a flush without motifs has a total of 0.
 * inq_motif_runs: the kernel alone over host buffers in exactly the format inq_read_seqs_fetch returns - n records, their packed
 * slices back to back in seq_bytes bytes -, with kept_off[n_loci + 1] telling which records belong to which locus (ascending,
 * kept_off[n_loci] <= n, else INQ_ERR_ARG; a record at or past kept_off[n_loci] has no locus and gets four zeros) and one motif word
 * per locus; out[n].  A record whose slice does not fit into seq_bytes gets four zeros. */
int inq_call_flush_motifs(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags,
                          inq_locus_evidence_t *evidence, uint64_t *kept_off, uint64_t *name_bytes, uint64_t *seq_bytes,
                          const uint64_t *motif /* [n_loci], host */);
int inq_read_motifs_fetch(inq_ctx_t *ctx, inq_read_motif_t *recs, uint64_t n);
int inq_motif_runs(inq_ctx_t *ctx, const inq_read_seq_t *recs, uint64_t n, const uint8_t *packed, uint64_t seq_bytes,
                   const uint64_t *kept_off /* [n_loci + 1] */, const uint64_t *motif /* [n_loci] */, uint64_t n_loci,
                   inq_read_motif_t *out);
/* records per workgroup and turn of the motif kernel (a constant of the build) */
uint32_t inq_read_motif_tile(void);
/* The motif each locus's kept reads repeat (inq_locus_motif_t above), found on the device at flush time out of the batch's own slices and
 * handed to the motif kernel of the same flush without a host round trip.  inq_call_flush_locus_motifs is inq_call_flush_motifs plus
 * `found`, a HOST array of n_loci records in append order.  found NULL = exactly inq_call_flush_motifs.  With it, seq_bytes NULL is
 * INQ_ERR_ARG; `motif` may be NULL (no locus has a given word); the read-motif records are produced for EVERY kept record, locus j
 * measured with motif[j] where that names a motif and with found[j].word where not, and inq_read_motifs_fetch works as after a flush
 * with motifs.
 * inq_locus_motifs_find: the kernel alone over host buffers in the format inq_read_seqs_fetch returns, as inq_motif_runs takes them
 * (same argument checks; kept_off must not be NULL, found not when n_loci != 0).  given: one word per locus or NULL; use: NULL, or
 * [n_loci] receiving what the motif kernel would be handed (given[j] where it names a motif, else found[j].word).  A record whose
 * slice does not fit into seq_bytes contributes nothing. */
int inq_call_flush_locus_motifs(inq_ctx_t *ctx, inq_result_t *result, uint64_t n_loci, double *ms_call, uint8_t *locus_flags,
                                inq_locus_evidence_t *evidence, uint64_t *kept_off, uint64_t *name_bytes, uint64_t *seq_bytes,
                                const uint64_t *motif /* [n_loci], host, may be NULL */, inq_locus_motif_t *found /* [n_loci], host */);
int inq_locus_motifs_find(inq_ctx_t *ctx, const inq_read_seq_t *recs, uint64_t n, const uint8_t *packed, uint64_t seq_bytes,
                          const uint64_t *kept_off /* [n_loci + 1] */, uint64_t n_loci, const uint64_t *given /* [n_loci] or NULL */,
                          inq_locus_motif_t *found /* [n_loci] */, uint64_t *use /* [n_loci] or NULL */);
/* Row arrays in device memory for a host that does not link the HIP runtime itself: n f64, filled with quiet NaN (a locus no span
 * holds prints NaN NaN); plain synchronous copies in and out. */
int inq_dev_alloc_rows(inq_ctx_t *ctx, uint64_t n, double **out);
void inq_dev_free_rows(inq_ctx_t *ctx, double *p);
int inq_dev_write_rows(inq_ctx_t *ctx, double *dst_device, const double *src_host, uint64_t n);
int inq_dev_read_rows(inq_ctx_t *ctx, double *dst_host, const double *src_device, uint64_t n);
uint64_t inq_call_deferred_loci(const inq_ctx_t *ctx); /* loci appended since the last flush */
void inq_call_discard(inq_ctx_t *ctx); /* forgets what was appended (a run that failed between two flushes; a flush, failed or not, does it too) */

/* Test / debug: copies the batch the last inq_call_span (or inq_call_flush) built on the device into caller-allocated HOST
 * arrays sized from that call's stats: cigar[n_cigar_words], reads[n_reads], pair_read[n_pairs],
 * locus_pair_off[n_loci + 1].  Any pointer may be NULL. */
int inq_span_fetch_batch(inq_ctx_t *ctx, uint32_t *cigar, inq_read_t *reads, uint32_t *pair_read, uint64_t *locus_pair_off);

/* ==== `inquiSTR outlier` (src/outlier.rs): outlying samples per locus of a combined .inq ====
 * values: HOST, row-major [n_rows][stride] f32, row i holding row_len[i] <= stride parsed numbers (NaN allowed:
 * get_repeat_lengths maps it to 0, src/outlier.rs:80-83).  method: z-score (std_deviation_and_mean + z_score_outliers,
 * :18-31, 97-110; f32 with the reference's sequential summation order) or DBSCAN (dbscan_outliers + mode, :112-145;
 * eps = max(2 * mode, 10), min points = mincluster, at most 8192 values per row).  flags[i][k] = 1 where
 * samples[k] is reported for row i; keep[i] tells what became of the row. */
#define INQ_OUTLIER_ZSCORE 0
#define INQ_OUTLIER_DBSCAN 1
#define INQ_OUTLIER_ROW_SKIP 0     /* max < minsize: get_repeat_lengths returns None, the row is not looked at      */
#define INQ_OUTLIER_ROW_KEEP 1
#define INQ_OUTLIER_ROW_EMPTY 2    /* no values: the reference panics (unwrap on None, src/outlier.rs:90)            */
#define INQ_OUTLIER_ROW_NO_MODE 3  /* DBSCAN, no value > 0: the reference panics ("No mode found for repeat", :144) */
#define INQ_OUTLIER_ROW_TOO_WIDE 4 /* DBSCAN row with more than 8192 values: not supported                           */
int inq_outlier_rows(inq_ctx_t *ctx, const float *values, const uint32_t *row_len, uint64_t n_rows, uint32_t stride,
                     int method, uint32_t minsize, float zscore_cutoff, uint32_t mincluster, uint8_t *flags,
                     uint8_t *keep);

/* ==== `inquistr assoc` (the reference's scripts/STR_regression.R): one regression per locus ====
 * values: HOST, row-major [n_rows][2 * n_samples] f32, the H1 / H2 of a sample side by side as a combined .inq holds them
 * (NaN = no call).  y[n_samples], cov[k][n_samples]: HOST f64, finite, shared by every row; binary y is 0 (group 1) or 1
 * (group 2), anything else INQ_ERR_ARG.  n_samples <= 65 535 and k <= 6, else INQ_ERR_ARG before any launch.
 * Per sample x = max / min / mean of the two haplotypes, one missing: the other, both: missing (that sample is left out of
 * this row).  Row filters, in this order: call rate n / n_samples >= missing_cutoff, more than one distinct x, both groups
 * there (binary), n > p = 2 + k.  Model [1, x, cov...]: binary = logistic regression by R's glm.fit iteration (start
 * mu = (y + 0.5) / 2, at most 25 steps, |dev - dev_old| / (|dev| + 0.1) < 1e-8, no step halving; Wald z, p = erfc(|z| / sqrt 2)),
 * continuous = least squares (t with n - p degrees of freedom, two-sided Student t).  Only x's coefficient is reported.
 * A pivot of the Cholesky factor of the centred normal equations at or below 1e-11 x their largest diagonal: SINGULAR.
 *
 * inq_assoc_row_t is 88 bytes: beta 0, se 8, stat 16, p 24, mean_all 32, mean_g1 40, mean_g2 48, min_x 56, max_x 64, n 72,
 * n_g1 76, n_g2 80, status 84, n_iter 85, pad 86.  n, the means and min / max are over the samples with an x (NaN without
 * one); the group fields are 0 / NaN for a continuous outcome; beta, se, stat, p are NaN unless status is OK or
 * NOT_CONVERGED (which carries the last iterate); n_iter = glm.fit's iteration count (0: continuous, or no fit). */
#define INQ_ASSOC_BINARY 0
#define INQ_ASSOC_CONTINUOUS 1
#define INQ_ASSOC_MAX 0
#define INQ_ASSOC_MIN 1
#define INQ_ASSOC_MEAN 2
#define INQ_ASSOC_ROW_OK 0
#define INQ_ASSOC_ROW_LOW_CALL_RATE 1
#define INQ_ASSOC_ROW_CONSTANT 2
#define INQ_ASSOC_ROW_ONE_GROUP 3
#define INQ_ASSOC_ROW_TOO_FEW 4
#define INQ_ASSOC_ROW_SINGULAR 5
#define INQ_ASSOC_ROW_NOT_CONVERGED 6
typedef struct inq_assoc_row {
    double beta, se, stat, p, mean_all, mean_g1, mean_g2, min_x, max_x;
    uint32_t n, n_g1, n_g2;
    uint8_t status, n_iter;
    uint8_t pad[2];
} inq_assoc_row_t;
int inq_assoc_rows(inq_ctx_t *ctx, const float *values, uint64_t n_rows, uint32_t n_samples, const double *y,
                   const double *cov, uint32_t k, int outcome, int str_mode, double missing_cutoff, inq_assoc_row_t *rows);

/* ---- Firth's penalised logistic regression for the rows whose maximum-likelihood fit breaks down ----
 * inq_assoc_rows for a binary outcome (rows[] gets the same bytes), and behind it, on the device, Firth's fit of the rows that
 * `when` selects: ALWAYS = every row whose status is OK or NOT_CONVERGED; FALLBACK = of those the NOT_CONVERGED ones and the ones
 * whose ordinary fit left min over the kept samples of min(mu, 1 - mu) below 1e-6 at its last pass (separation that stopped on the
 * deviance; the bound is the context option "assoc_firth_mu_ppb", in units of 1e-9, default 1000).  Any other `when`: INQ_ERR_ARG
 * before any launch.  Limits, tiling ("assoc_tile_rows") and the other argument errors are those of inq_assoc_rows.
 * The model: columns, centring, x, rank tolerance and the mu clamp of the ordinary fit.  With pi = 1 / (1 + exp(-eta)),
 * w = pi (1 - pi), I = X'WX: penalised log-likelihood l* = sum [y log pi + (1 - y) log(1 - pi)] + 1/2 log det I, hat values
 * h_i = w_i x_i' I^-1 x_i, modified score U* = sum (y - pi + h (1/2 - pi)) x_i.  From beta = 0: evaluate I, U*, l* at beta and
 * delta = I^-1 U* over the free coefficients; stop, OK, when max_j |delta_j| sqrt(I_jj) < 1e-9 (beta as it stands is the
 * estimate); else scale delta to max_j |delta_j| <= 5, beta += delta.  No step halving.  A non-finite l*, or no stop at the
 * evaluation after 100 steps: NOT_CONVERGED with the last iterate.  A failed pivot at any evaluation: SINGULAR, numbers NaN.
 * Full fit: all p coefficients free.  Null fit: beta_x held at 0, the others free, h and log det I from the full p x p matrix.
 * beta = beta_x of the full fit, se = sqrt((I^-1)_xx) there, chi2 = max(0, 2 (pll_full - pll_null)), p = erfc(sqrt(chi2 / 2))
 * (one degree of freedom); n_iter_* = steps taken.  The row's status is the worse of its two fits'.
 *
 * inq_assoc_firth_row_t is 56 bytes: beta 0, se 8, chi2 16, p 24, pll_full 32, pll_null 40, n_iter_full 48, n_iter_null 49,
 * status 50, pad 51.  A row that is not fitted: NOT_FITTED, numbers NaN, counts 0. */
#define INQ_ASSOC_FIRTH_FALLBACK 1
#define INQ_ASSOC_FIRTH_ALWAYS 2
#define INQ_ASSOC_FIRTH_ROW_OK 0
#define INQ_ASSOC_FIRTH_ROW_NOT_FITTED 1
#define INQ_ASSOC_FIRTH_ROW_SINGULAR 2
#define INQ_ASSOC_FIRTH_ROW_NOT_CONVERGED 3
typedef struct inq_assoc_firth_row {
    double beta, se, chi2, p, pll_full, pll_null;
    uint8_t n_iter_full, n_iter_null, status;
    uint8_t pad[5];
} inq_assoc_firth_row_t;
int inq_assoc_rows_firth(inq_ctx_t *ctx, const float *values, uint64_t n_rows, uint32_t n_samples, const double *y,
                         const double *cov, uint32_t k, int str_mode, double missing_cutoff, int when, inq_assoc_row_t *rows,
                         inq_assoc_firth_row_t *firth);

const char *inq_strerror(int code);
const char *inq_backend_name(const inq_ctx_t *ctx); /* "hip:gfx950:<device name>" */
const char *inq_last_error(const inq_ctx_t *ctx);   /* detail of the last INQ_ERR_HIP */
int inq_abi_version(void);
/* NUMA node of the host the context's GPU hangs off (its PCI address through sysfs), -1 if unknown: a host buffer the GPU's
 * copy engine reads is best placed there (268 MB from the other socket: 5.6 - 6.1 ms instead of 4.9 ms on the boxes measured). */
int inq_ctx_numa_node(const inq_ctx_t *ctx);

#ifdef __cplusplus
}
#endif
#endif /* INQUISTR_HIP_H */
