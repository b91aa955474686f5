// inq_text.h — the text side of `inquiSTR call`: .inq rows, header, sample name, output order.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/inquistr_hip.h"  // inq_locus_evidence_t, inq_read_call_t

namespace inqhost {

// Rust `{}` of an f64 that is an integer, a half, or NaN (src/call.rs:57-65 prints phase1/phase2 so)
std::string format_f64(double v);
// Genotype Display, src/call.rs:57-65
// bare-pointer form of append_row for the output stage; returns the end.  dst needs chrom.size() + kRowBytesMax bytes.
constexpr size_t kRowBytesMax = 4 + 2 * 10 + 2 * 320;
char *write_row(char *dst, const std::string &chrom, uint32_t start, uint32_t end, double p1, double p2);
std::string format_row(const std::string &chrom, uint32_t start, uint32_t end, double p1, double p2);
// the same, appended to a growing buffer (no temporaries: the output of 10^5 .. 10^6 rows is on the critical path)
void append_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, double p1, double p2);
void append_f64(std::string &out, double v);
// src/call.rs:101
std::string format_header(const std::string &sample);
// the evidence file (inq_call_args_t::evidence_path; not a reference output): its header, and the line of one target
extern const char *const kEvidenceHeader;
void append_evidence_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_locus_evidence_t &e);
// the read-calls file (inq_genotype_repeats_reads; not a reference output): its header, and the line of one target from the records of its
// kept reads in file order - h1 / h2 are the Calls median_str_length is handed for phase1 / phase2, ascending by (value, file order)
extern const char *const kReadCallsHeader;
void append_read_calls_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls, size_t n,
                           bool unphased);
// the read table (inq_genotype_repeats_table; not a reference output): its header, and the lines of one target - one per kept read, in the
// order of the read-calls lists (h1 in that list's order, then h2, then other) - from the records, their origins (same order) and
// their names back to back (record k's name: name_len bytes behind the names of the records in front of it).  A name is cut at its
// first NUL, an empty one printed as `*`; the bytes go out as they stand (SAM keeps tab and newline out of a QNAME: [!-?A-~]).
// Every line ends in a newline; a target without a kept read appends nothing.
extern const char *const kReadTableHeader;
void append_read_table_rows(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                            const inq_read_origin_t *origins, const uint8_t *names, size_t n, bool unphased);
// the read-seqs file (inq_genotype_repeats_seqs; not a reference output): its header, and the lines of one target - those of the read
// table in columns chrom .. read, then qbeg, len and the bases of the read's SEQ over the locus window (inq_read_seq_t of
// include/inquistr_hip.h: seqs in the records' order, their packed slices back to back, (n_bases + 1) / 2 bytes each); `*` for an empty one
extern const char *const kReadSeqsHeader;
void append_read_seq_rows(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                          const inq_read_origin_t *origins, const uint8_t *names, const inq_read_seq_t *seqs, const uint8_t *packed, size_t n,
                          bool unphased);
// The slice contract of inq_read_seq_t as a plain sequential CIGAR walk: what the host sweep cuts with (inq_host_seq_window)
void seq_window(const uint32_t *cigar, uint32_t n_cigar, int32_t pos, uint32_t l_seq, uint32_t start, uint32_t end, uint32_t *q_beg,
                uint32_t *n_bases);
// bases [q_beg, q_beg + n_bases) of a BAM SEQ field appended to out, packed from the high nibble of a fresh byte on
void pack_seq_slice(const uint8_t *seq, uint32_t q_beg, uint32_t n_bases, std::vector<uint8_t> &out);
// The motif word of inq_read_motif_t (include/inquistr_hip.h) from a motif's text: upper-cased, A C G T only, reduced to its primitive
// root, 1 .. 15 bases.  0 and the word, else *word = 0 and kMotifEmpty / kMotifLetter / kMotifLong
enum { kMotifOk = 0, kMotifEmpty = 1, kMotifLetter = 2, kMotifLong = 3 };
int motif_encode(const char *text, uint64_t *word);
// the word's motif as text, `.` for a word that is no motif
std::string motif_text(uint64_t word);
// The run contract of inq_read_motif_t as a plain sequential walk, a rotation at a time, over n_bases packed bases (first base in the
// high nibble of the first byte): what the host sweep computes with (inq_host_motif_runs)
void motif_runs(const uint8_t *packed, uint32_t n_bases, uint64_t word, inq_read_motif_t *out);
// the read-motifs file (inq_genotype_repeats_motifs; not a reference output): its header, and the lines of one target - those of the
// read-seqs file in columns chrom .. len, then the target's motif, run_beg, run_len, units = run_len / k, motif_bases and runs of each
// record's inq_read_motif_t; a target whose word is no motif prints `.` in all six
extern const char *const kReadMotifsHeader;
void append_read_motif_rows(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, const inq_read_call_t *calls,
                            const inq_read_origin_t *origins, const uint8_t *names, const inq_read_seq_t *seqs, const inq_read_motif_t *motifs,
                            uint64_t word, size_t n, bool unphased);
// The motif a locus's kept reads repeat, inq_locus_motif_t of include/inquistr_hip.h, restated as a plain sequential walk, base by base,
// over the locus's n_records slices packed back to back (each from a fresh byte on, n_bases[r] bases): what the host sweep computes
// with (inq_host_locus_motif_find)
void locus_motif_find(const uint8_t *packed, const uint32_t *n_bases, size_t n_records, inq_locus_motif_t *out);
// the word a locus's runs are measured with when the motifs are looked for: the given one where it names a motif, else the found one
// (what locus_motif_kernel writes to `use`)
uint64_t motif_word_in_use(uint64_t given, uint64_t found);
// the locus-motifs file (inq_genotype_repeats_locus_motifs; not a reference output): its header, and one target's line -
// `chrom begin end reads bases motif period tandem copies catalogue agrees`, motif and catalogue as motif_text of the found and of the
// catalogue's word, agrees 1 / 0 where the catalogue's word names a motif and is / is not a rotation of the found one (none found: 0),
// `.` where it names none.  Returns what it printed there: 1, 0, or -1 for `.`
extern const char *const kLocusMotifsHeader;
int append_locus_motif_row(std::string &out, const std::string &chrom, uint32_t start, uint32_t end, uint64_t reads, const inq_locus_motif_t &found,
                           uint64_t catalogue_word);
// src/call.rs:91-100: file_stem, then every ".bam" and ".cram" removed
std::string sample_name_from_path(const std::string &bam_path);
// [3P] human_sort::compare as used by Genotype::cmp (src/call.rs:33-38): <0, 0, >0
int human_compare(const std::string &a, const std::string &b);

}  // namespace inqhost
