/*
 * dskgpu.h -- C-ABI of the MI355X k-mer counting engine (libdskgpu.so).
 *
 * This is the drop-in boundary for the DSK count path.  In the reference the
 * whole path is ONE C++ call, `SortingCountAlgorithm<span>::execute()`
 * (src/DSK.cpp:55-60), fed by `Bank::open(-file)` (src/DSK.cpp:51) and read
 * back through `Partition<Kmer<span>::Count> "solid"` + the histogram
 * (utils/dsk2ascii.cpp:61-104; scripts/simple_test.sh:37).  The reference has
 * no FFI of its own (it is all in-process C++), so each entry point below cites
 * the reference interface it stands in for.  Plain pointers and sizes only; no
 * C++/torch types cross.  Every function returns DSKGPU_OK (0) or a negative
 * error code; `dskgpu_last_error` gives the text.  One ctx per device; a ctx
 * is not thread-safe, distinct ctxs are independent.
 *
 * Input convention ("read stream"): a byte string in which every maximal run
 * of [ACGTacgt] is one sequence fragment; ANY other byte (N, IUPAC codes,
 * '\n' between reads) ends the current k-mer window (test/readN.fasta +
 * test/readN.histo).  A bank front-end therefore only has to concatenate the
 * sequence lines of its records separated by one non-ACGT byte -- or hand over
 * the file's text as it is and let the device do that (dskgpu_push_raw).
 *
 * K-mer value convention (README.md:104-112, utils/dsk2ascii.cpp:104): A=0,
 * C=1, T=2, G=3, first base most significant; canonical = min(fwd, revcomp).
 * A k-mer is `words` = ceil(k / 32) 64-bit words, least-significant word first
 * (1 for k <= 32, 2 for k <= 64, 3 for k <= 96, 4 for k <= 128).
 */
#ifndef DSKGPU_H
#define DSKGPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSKGPU_OK 0
#define DSKGPU_E_ARG (-1)       /* bad argument / unsupported k            */
#define DSKGPU_E_DEVICE (-2)    /* HIP error (text in dskgpu_last_error)   */
#define DSKGPU_E_NOMEM (-3)     /* device allocation failed                */
#define DSKGPU_E_STATE (-4)     /* call out of order                       */
#define DSKGPU_E_OVERFLOW (-5)  /* internal table overflow after retries   */
#define DSKGPU_E_FORMAT (-6)    /* dskgpu_push_raw: the text is not what was declared (see there)            */
#define DSKGPU_NOT_RESERVED 1   /* dskgpu_reserve_work only: nothing was reserved (the request exceeds 60 % of the free HBM) -- not an
                                   error: dskgpu_count sizes its own buffers, in several passes if need be; nothing was allocated */

typedef struct dskgpu_ctx dskgpu_ctx;

/* Options of SortingCountAlgorithm<>::getOptionsParser() that reach the
 * count path (src/DSK.cpp:83; README.md:12,56; scripts/simple_test.sh:36,88). */
typedef struct dskgpu_config {
    uint32_t kmer_size;       /* -kmer-size, 1..128 (gatb spans 32/64/96/128 serve k < span; README.md:115-122, CMakeLists.txt:42) */
    uint32_t abundance_min;   /* -abundance-min (solid <=> min <= count <= max) */
    uint32_t abundance_max;   /* -abundance-max                                */
    uint32_t histo_max;       /* -histo-max: histogram rows 1..histo_max (10000) */
    int32_t  device;          /* HIP device ordinal                            */
    uint32_t nb_partitions;   /* number of output partitions (dsk/solid/<p>); 0 = auto */
    uint32_t minimizer_size;  /* -minimizer-size (used by the owner map), 0 = default 10 */
    uint32_t flags;           /* DSKGPU_F_* */
    uint32_t world_size;      /* number of GPUs sharing the k-mer space (1 = single) */
    uint32_t rank;            /* this GPU's index in [0, world_size)           */
    uint32_t max_pass_mkeys;  /* most k-mers (in millions) one pass may hold; 0 = 4026 (32-bit offsets).
                                 Larger inputs are counted in several passes over the key space, the
                                 in-HBM counterpart of DSK's disk passes (README.md:126-130) */
    uint32_t solidity_kind;   /* DSKGPU_SOLIDITY_*: how the counts of several banks decide solidity (-solidity-kind) */
    uint32_t solidity_custom; /* DSKGPU_SOLIDITY_CUSTOM: bit b set = bank b must hold the k-mer (-solidity-custom) */
    uint32_t reserved[3];
} dskgpu_config;

#define DSKGPU_F_TIMING 1u        /* record per-stage HIP-event timings        */
#define DSKGPU_F_NO_SORT 2u       /* leave solid rows unsorted (bench ablation) */
#define DSKGPU_F_MG_EXPLICIT 8u   /* multi-GPU: exchange one explicit key per k-mer instead of super-k-mer records */
#define DSKGPU_F_HISTO2D 4u       /* also build the 2-D histogram: bank 0 (genome) x the other banks (reads), -histo2D */
#define DSKGPU_F_PARTITION_ORDER 32u /* the REFERENCE's row order instead of the global one: rows ascending inside an output partition, partitions = runs of
                                   * hash sub-partitions of at most 4096 rows (dskgpu_num_partitions of them: thousands) -- what Partition<Count> "solid"
                                   * guarantees its readers (utils/dsk2ascii.cpp:61,77,85-104: partition after partition, the rows of each as they
                                   * come; gatb-core's partitions are classes of the minimizer hash).  One pass over the rows instead of three
                                   * (csrc/partsort.h).  Honoured at every k (1 <= k <= 128), by a single pass and by every pass of a multi-pass count;
                                   * rows per partition: at most 4096 (PS_CAP) for k <= 32, 2048 (PS2_CAP) for 33 <= k <= 64, 1024 (PS4_CAP) for
                                   * 65 <= k <= 128 (four-word device keys: one 36-byte row per thread of the block that orders the partition).  The
                                   * per-bank modes (a solidity kind other than sum, DSKGPU_F_HISTO2D) -- and an input on which a partition would
                                   * exceed what one block orders -- keep the global order, which satisfies the same contract with nb_partitions
                                   * value ranges. */
#define DSKGPU_F_PLACE 16u        /* pick the place of every big device buffer: where a buffer lies in HBM changes the rate of
                                   * scattered stores into it by up to 40 % (tools/micro/write_place.hip; the "two speeds" of the
                                   * partition kernels).  Each allocation >= 256 MB becomes the best of up to 8 candidates, timed
                                   * with the store pattern of the level-1 scatter; the others are freed.  One-off cost at the
                                   * first count (~3-6 s for 30 GB of buffers): for contexts that count many times.  Process-wide
                                   * once a context asked for it; DSKGPU_PLACE=<candidates> in the environment does the same. */

/* -solidity-kind (gatb-core option; only `sum` is exercised by the reference's tests, README.md:12).
 * Banks = the inputs separated with dskgpu_next_bank / dskgpu_set_banks; one bank => plain counting. */
#define DSKGPU_SOLIDITY_SUM 0u    /* amin <= sum of the banks' counts <= amax (default)            */
#define DSKGPU_SOLIDITY_MIN 1u    /* amin <= smallest per-bank count <= amax                       */
#define DSKGPU_SOLIDITY_MAX 2u    /* amin <= largest per-bank count <= amax                        */
#define DSKGPU_SOLIDITY_ONE 3u    /* at least one bank has amin <= count <= amax                   */
#define DSKGPU_SOLIDITY_ALL 4u    /* every bank has amin <= count <= amax                          */
#define DSKGPU_SOLIDITY_CUSTOM 5u /* banks in solidity_custom have count >= amin, the others 0     */

/* Lifetime: stands where `SortingCountAlgorithm<span> sortingCount(bank, props)`
 * is constructed / destroyed (src/DSK.cpp:55). */
int  dskgpu_create(const dskgpu_config* cfg, dskgpu_ctx** out);
void dskgpu_destroy(dskgpu_ctx* ctx);
const char* dskgpu_last_error(const dskgpu_ctx* ctx);   /* ctx may be NULL: create-time error */
const char* dskgpu_version(void);
int dskgpu_device_count(void);                          /* HIP devices visible to this process (0 when there is none) */

/* Launch all device work of this ctx on an existing HIP stream (hipStream_t
 * passed as void*); NULL = a stream owned by the ctx. */
int dskgpu_set_stream(dskgpu_ctx* ctx, void* hip_stream);

/* ---- input: replaces the Bank iteration inside execute() (src/DSK.cpp:51,60) */
/* Append host bytes of the read stream (copied to the device; may be called
 * repeatedly; a separator is implied between calls).  `bytes` may be reused as soon as the call returns (it is staged), but the
 * DMA to the device may still be in flight then: an asynchronous copy error is reported by the next call that synchronises
 * (dskgpu_count, dskgpu_encode_reads, dskgpu_set_stream, a buffer growth), not by this one. */
int dskgpu_push_reads(dskgpu_ctx* ctx, const char* bytes, uint64_t nbytes);
/* Append FILE TEXT -- FASTA or FASTQ exactly as it lies in the (inflated) file, headers and quality lines included -- and let the
 * device turn it into the read stream: replaces BankFasta's parser (gatb-core BankFasta behind src/DSK.cpp:51 Bank::open; the
 * formats of README.md:52-61) together with dskgpu_push_reads' clean stream.  The text may be cut ANYWHERE between calls (mid
 * line, mid record): the parser's state is kept on the device.  `new_file` != 0 says that `text` begins a new file (line
 * counting restarts, the records of two files never join); the first raw push of a read set is a new file by itself.
 *   DSKGPU_RAW_FASTQ  four lines per record ('@' header, sequence, '+' line, qualities): the sequence lines are kept
 *   DSKGPU_RAW_FASTA  '>' header lines are dropped, all other lines are sequence, joined when a record is wrapped over lines
 * Asynchronous like dskgpu_push_reads: nothing is known about the result until something needs the stream's length -- every
 * call that reads the reads (dskgpu_count, dskgpu_encode_reads, dskgpu_mg_*, dskgpu_next_bank, dskgpu_push_reads) first does
 * what dskgpu_raw_finish does.  A text the device parser does not handle (a FASTQ file with sequences wrapped over several
 * lines or blanks inside them, one whose quality lines do not add up to its sequence lines -- a host parser reads as many
 * quality characters as the record has bases --, text that is neither format) is DETECTED, never mis-parsed: dskgpu_raw_finish returns
 * DSKGPU_E_FORMAT and the stream is what it was before the raw pushes -- the caller parses on the host and pushes the reads. */
#define DSKGPU_RAW_FASTA 1
#define DSKGPU_RAW_FASTQ 2
int dskgpu_push_raw(dskgpu_ctx* ctx, const char* text, uint64_t nbytes, int format, int new_file);
/* Wait for the raw pushes; -> the read stream's length in bytes and the number of records (header lines) the raw pushes since the
 * last finish held -- Bank::estimate's sequence count (both may be NULL). */
int dskgpu_raw_finish(dskgpu_ctx* ctx, uint64_t* stream_bytes, uint64_t* records);
/* The length of the pushed read stream in bytes (waits for raw pushes), and its rewind: the stream is cut back to its first
 * `stream_bytes` bytes -- what was pushed behind them is forgotten (a bank front-end that parsed a damaged file in parallel and
 * found out that a serial parse would differ pushes that file again; src/DSK.cpp:51: the reference's parser is serial). */
int dskgpu_stream_bytes(dskgpu_ctx* ctx, uint64_t* stream_bytes);
int dskgpu_rewind_reads(dskgpu_ctx* ctx, uint64_t stream_bytes);
/* Optional: size the device-side read buffer once (e.g. from Bank::getSize) instead of growing it push by push. */
int dskgpu_reserve_reads(dskgpu_ctx* ctx, uint64_t nbytes);
/* Optional: allocate the partition buffers of a count over up to `nbytes` read-stream bytes now (tens of GB of HBM: 0.2 s of
 * hipMalloc on a 10 M-read input) instead of inside the first dskgpu_count.  May run on another host thread WHILE the reads
 * are pushed -- it touches nothing dskgpu_push_reads / dskgpu_reserve_reads use -- but must have returned before dskgpu_count.
 * Call order: before dskgpu_encode_reads or never -- after it the kept encoding is the only copy of the reads, and this call
 * then leaves the encoded stream's buffers as they are (it only sizes the partition buffers).
 * Stands where SortingCountAlgorithm's configure step sizes its passes and partitions before execute() fills them. */
int dskgpu_reserve_work(dskgpu_ctx* ctx, uint64_t nbytes);   /* DSKGPU_OK, DSKGPU_NOT_RESERVED (a soft refusal, see above), or an error */
/* Use a read stream already resident in HBM (caller keeps ownership and must
 * keep it alive until dskgpu_count returns).  Replaces any pushed reads.  The call waits for all device work this
 * process has submitted so far (hipDeviceSynchronize): bytes that another stream is still writing when it is made
 * are complete when it returns.  Bytes written AFTER the call must be ordered by the caller (same stream as
 * dskgpu_set_stream, or a synchronisation of its own) before dskgpu_count. */
int dskgpu_set_reads_device(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes);

/* Optional: turn the current reads into their 2-bit form NOW (the first stage of every count: 0.375 bytes per base) and let go of
 * the bytes: a device-resident stream handed over with dskgpu_set_reads_device is never read again after this call returns -- the
 * caller may free or overwrite it --, reads that were pushed lose their copy in HBM.  Every later dskgpu_count / dskgpu_mg_* of
 * these reads starts from the kept encoding.  For inputs whose ASCII form would crowd the partitions out of HBM: 90 Gbp of reads
 * are 90 GB as bytes and 34 GB encoded, and the difference decides how many sweeps over the reads a multi-pass count needs
 * (README.md:126-130: DSK reads its bank once per pass and keeps nothing of it in memory).  Not with per-bank modes
 * (-solidity-kind other than sum, -histo2D), which re-read bank by bank: DSKGPU_E_STATE there.  A new dskgpu_push_reads /
 * dskgpu_set_reads_device starts a new read set. */
int dskgpu_encode_reads(dskgpu_ctx* ctx);

/* Banks: the comma-separated inputs of `-file` are separate banks (README.md:52-58).  Call
 * dskgpu_next_bank between the pushes of two banks (or behind every bank, the last one too: a bank may be EMPTY -- a file without
 * reads, a rank's empty share of a small bank -- and is only known to exist by its call), or give the end offset of every bank of a
 * device-resident stream.  Only needed for -solidity-kind != sum and -histo2D; at most 32 banks. */
int dskgpu_next_bank(dskgpu_ctx* ctx);
int dskgpu_set_banks(dskgpu_ctx* ctx, const uint64_t* end_offsets, uint32_t n_banks);

/* ---- the hot path: replaces SortingCountAlgorithm<span>::execute() (src/DSK.cpp:60) */
/* Single-GPU: encode -> canonical k-mers -> partition -> count -> histogram +
 * solidity filter (+ sort).  Synchronous on return. */
int dskgpu_count(dskgpu_ctx* ctx);

/* Multi-GPU (world_size > 1): the k-mer space is split over owners in [0, world_size).  The owner of a
 * k-mer is a function of the MINIMIZER of its window (m = minimizer_size), so runs of consecutive k-mers
 * share an owner and travel as one super-k-mer record of 2-bit packed bases (2-3 words for up to 16
 * k-mers) -- DSK v2's minimizer repartition + super-k-mers (CHANGELOG.md:13) used as the wire format.
 * For k < 20 or with DSKGPU_F_MG_EXPLICIT the records are explicit keys (1-2 words per k-mer, owner =
 * a bit field of the mixed k-mer).  Step 1 writes this rank's records grouped by owner into caller
 * memory `d_send` (capacity in 8-byte words) and the per-owner word counts into send_words[world_size]
 * (host).  The caller exchanges the groups (RCCL all-to-all) and hands the received words to step 2.
 * dskgpu_mg_send_capacity_words runs the sizing pass over the current reads and returns the words
 * dskgpu_mg_scatter will need (0 on error). */
int dskgpu_mg_scatter(dskgpu_ctx* ctx, void* d_send, uint64_t capacity_words, uint64_t* send_words);
/* Minimizer repartition (gatb-core's RepartitorAlgorithm; the call site that reads its result is src/DSK.cpp:63 getConfig):
 * the owner of a window = table[bucket of its minimizer], DSKGPU_MG_BUCKETS buckets.  Default: the bucket scaled to
 * world_size.  A balanced table comes from sampled loads: every rank calls dskgpu_mg_sample on its reads (k-mers per bucket,
 * estimated from every 16th tile), the loads are summed over the ranks (an all-reduce of 32 KB), dskgpu_mg_make_table turns
 * the sum into a table -- deterministic, so every rank computes the same one -- and dskgpu_mg_set_table installs it before
 * dskgpu_mg_scatter.  A bucket holding more than a quarter of a fair share (poly-A, microsatellite minimizers) gets
 * DSKGPU_MG_SPLIT: its windows go to the owner of their own k-mer as one-k-mer records; the others are placed largest first
 * on the least loaded owner.  The table must be the same on every rank; results never depend on which table is used.
 * (dskgpu_group_count does all of this by itself.) */
#define DSKGPU_MG_BUCKETS 4096
#define DSKGPU_MG_SPLIT 255
int dskgpu_mg_sample(dskgpu_ctx* ctx, uint64_t* loads /* [DSKGPU_MG_BUCKETS] */);
void dskgpu_mg_make_table(const uint64_t* summed_loads, uint32_t world_size, uint8_t* table /* [DSKGPU_MG_BUCKETS] */);
int dskgpu_mg_set_table(dskgpu_ctx* ctx, const uint8_t* table /* [DSKGPU_MG_BUCKETS], NULL = default */);
uint64_t dskgpu_mg_send_capacity_words(dskgpu_ctx* ctx);
int dskgpu_mg_count(dskgpu_ctx* ctx, const void* d_recv, uint64_t recv_words);
/* The senders know how many k-mers they packed for every owner (counted while the records are written):
 * dskgpu_mg_sent_kmers returns that row after dskgpu_mg_scatter (host array of world_size entries), the caller sends it
 * along with the word counts, and the receiver passes the column sum to dskgpu_mg_count_sized -- which then skips its own
 * pass over the received records (0.6 ms of a 20 ms step).  n_kmers = 0 behaves as dskgpu_mg_count; a figure that does not
 * match the records is reported as DSKGPU_E_ARG, never as a wrong result. */
int dskgpu_mg_sent_kmers(dskgpu_ctx* ctx, uint64_t* kmers /* [world_size] */);
int dskgpu_mg_count_sized(dskgpu_ctx* ctx, const void* d_recv, uint64_t recv_words, uint64_t n_kmers);
/* ---- the same step in SLICES, so that the exchange overlaps both of its neighbours: the exchange of slice i runs while the
 * sender writes slice i + 1 and while the receiver partitions slice i - 1.  Needs the sampled send layout (its sizes are known
 * before a record exists: the word counts of ALL slices go round once, up front):
 *   dskgpu_mg_slices_prepare  sizing pass; *nslices = 0 when this input takes the one-piece path (small input, explicit keys, a
 *                             send slice overflowed before) -- then use dskgpu_mg_scatter / dskgpu_mg_count.  Otherwise
 *                             send_words[s * world_size + o] = words slice s holds for owner o (slice-major, owner-major inside: the
 *                             send buffer is the concatenation, dskgpu_mg_send_capacity_words in all), kmers_est[o] = estimated
 *                             k-mers for owner o over all slices (sizes the receiver; an estimate, never a correctness input).
 *   dskgpu_mg_scatter_slice   launches the sender of slice s on the context's stream and returns (no synchronisation): the caller
 *                             records an event behind it and starts that slice's exchange on another stream.
 *   dskgpu_mg_count_sliced    the receiver: d_recv holds the slices one after the other (slice_words[s] words each, whatever the
 *                             order of the sources inside a slice); gate(user, s) is called on the host right before the first
 *                             device work that reads slice s is enqueued -- the callee makes the context's stream wait for the
 *                             arrival of slice s (hipStreamWaitEvent / a torch work handle's wait()).  Slices are gated in order,
 *                             each once; a path that needs all records at once gates all of them first.  A gate that returns
 *                             non-zero (the wait failed: a collective timed out or was aborted) stops the count: no further device
 *                             work is enqueued, the remaining gates are still called (their result ignored), the call returns
 *                             DSKGPU_E_STATE and the context holds no result.
 *   dskgpu_mg_slices_finish   after the exchange: *overflowed != 0 when a slice of the SEND layout overflowed -- the records of this
 *                             step are then incomplete on some receivers, and every rank must repeat the step in one piece (the
 *                             decision is the caller's collective: OR the flags); the context will use exact counts from then on. */
typedef int (*dskgpu_slice_gate)(void* user, uint32_t slice);   /* 0 = the stream now waits for the slice; non-zero = it will never arrive */
int dskgpu_mg_slices_prepare(dskgpu_ctx* ctx, uint32_t want_slices, uint32_t* nslices, uint64_t* send_words /* [want_slices * world_size] */,
                             uint64_t* kmers_est /* [world_size] */);
int dskgpu_mg_scatter_slice(dskgpu_ctx* ctx, void* d_send, uint64_t capacity_words, uint32_t slice);
int dskgpu_mg_slices_finish(dskgpu_ctx* ctx, int* overflowed);
int dskgpu_mg_count_sliced(dskgpu_ctx* ctx, const void* d_recv, uint32_t nslices, const uint64_t* slice_words, uint64_t n_kmers_est,
                           dskgpu_slice_gate gate, void* user);

/* ---- results: replace the CountProcessor outputs read back through
 * Storage (src/DSK.cpp:68; utils/dsk2ascii.cpp:61-104; simple_test.sh:37) */
typedef struct dskgpu_stats {
    uint64_t n_bytes;        /* read-stream bytes processed              */
    uint64_t n_kmers;        /* valid k-mer occurrences                  */
    uint64_t n_distinct;     /* distinct canonical k-mers                */
    uint64_t n_solid;        /* rows passing the abundance filter        */
    uint32_t n_partitions;   /* output partitions                        */
    uint32_t n_levels;       /* radix-partition levels used              */
    uint32_t n_final_bins;   /* hash-aggregate sub-partitions            */
    uint32_t n_retries;      /* attempts repeated: a count table overflowed (finer plan), a sampled slice / the region pool overflowed (exact path), or (two-word keys) the top-word table met two k-mers with one top word (count stage again with full compares) */
    uint64_t sort_fallback;  /* 1 if the row sort needed its full-width fallback */
    uint64_t n_passes;       /* passes over the key space (1 unless the input exceeds a pass) */
    uint64_t n_ext_regions;  /* extension regions taken by sub-partitions that outgrew their home region (repeat-rich
                                inputs: heavy k-mers stay on the histogram-free path; 0 on repeat-free reads)   */
    uint64_t n_heavy;        /* k-mers counted apart from the partitions (found heavy in the sample pass)       */
    uint64_t n_read_sweeps;  /* times the (2-bit) reads were walked to generate k-mers: 1 for a single pass; a multi-pass
                                count materialises the keys of up to 16 passes per sweep -- this is what DSK calls a pass
                                (each one re-reads the input; README.md:126-130 "below 10")                             */
} dskgpu_stats;
/* The record of the last COUNT: dskgpu_filter_rows / dskgpu_clip_tips change neither it nor the histogram (n_solid stays what the count found). */
int dskgpu_get_stats(const dskgpu_ctx* ctx, dskgpu_stats* out);

/* out[0..nbins-1]; out[i] = number of distinct k-mers whose
 * min(count, histo_max) == i; nbins must be histo_max+1 (out[0] == 0).
 * Same content as the `histogram/histogram` dataset (test/k27.histo). */
int dskgpu_histogram(const dskgpu_ctx* ctx, uint64_t* out, uint32_t nbins);

/* 2-D histogram (flag DSKGPU_F_HISTO2D): out[r * 11 + g] = number of distinct k-mers seen min(r, histo_max)
 * times in the read banks (banks 1..) and min(g, 10) times in bank 0; nrows must be histo_max + 1.
 * Text form `<out>.histo2D` (README.md:98-102; utils/plot-histo2D.R:22-30). */
int dskgpu_histogram2d(const dskgpu_ctx* ctx, uint64_t* out, uint32_t nrows);

/* Output partitions = `Partition<Count> "solid"` (utils/dsk2ascii.cpp:61,77).
 * Rows are ascending by k-mer value inside a partition; by default the partitions are
 * ascending value ranges too, so the concatenation is globally sorted (with
 * DSKGPU_F_PARTITION_ORDER only the order inside a partition is guaranteed). */
/* Row order of the NEXT counts of this context: non-zero = DSKGPU_F_PARTITION_ORDER (see the flag), 0 = the global order. */
int dskgpu_set_row_order(dskgpu_ctx* ctx, int partition_order);
uint32_t dskgpu_num_partitions(const dskgpu_ctx* ctx);
uint64_t dskgpu_partition_size(const dskgpu_ctx* ctx, uint32_t p);
/* offsets[p] = first row of partition p in the result arrays (dskgpu_result_device), offsets[num_partitions] = all rows:
 * what a caller of DSKGPU_F_PARTITION_ORDER walks (thousands of partitions: one call instead of one per partition). */
int dskgpu_partition_offsets(const dskgpu_ctx* ctx, uint64_t* offsets /* [dskgpu_num_partitions + 1] */);
/* kmers: size*words u64 (row-major, LSW first, words = ceil(k/32)); abundance: size u32. Host memory. */
int dskgpu_partition_copy(const dskgpu_ctx* ctx, uint32_t p, uint64_t* kmers, uint32_t* abundance);
/* Device pointers to the full sorted result (valid until the next count/destroy).  d_kmers = word 0 of
 * every row; the device keeps one array per word (struct of arrays), higher words via dskgpu_partition_copy. */
int dskgpu_result_device(const dskgpu_ctx* ctx, const void** d_kmers, const void** d_abundance, uint64_t* n_rows);

/* Per-stage device time of the last count (flag DSKGPU_F_TIMING).  Returns the
 * number of stages; fills up to `cap` entries.  names[i] are static strings.  The lookups below add the stages "query index" and
 * "query" (summed over the calls since the last count). */
int dskgpu_stage_times(const dskgpu_ctx* ctx, const char** names, float* ms, int cap);

/* ---- lookups in the last result: what the readers of `Partition<Count> "solid"` do with a count next -- how often does this k-mer, or
 * every k-mer of this read, occur? (gatb-core's consumers iterate and probe the partitions; Jellyfish `query`, KMC `CheckKmer`).
 * On the device, for every k (1..128) and every result a context can hold: either row order, one pass or several, DSKGPU_F_NO_SORT,
 * the per-bank modes (the answer is whatever the row's abundance column holds), a rank's rows after dskgpu_mg_count* /
 * dskgpu_group_count.  A rank's rows are the solid k-mers that rank owns and every k-mer has one owner, so the answer of a GROUP is the
 * sum over the ranks of the per-rank answers, asked through dskgpu_group_ctx(g, r); there is no routed group query.
 * The index is one hash table over the rows in HBM (8 bytes per slot, 2 .. 4 slots per row: 16 .. 32 bytes per row), built by the
 * first query after a count or by dskgpu_query_prepare, dropped -- and its memory freed -- when the next count starts and by
 * dskgpu_destroy; a query after the next count answers from the new rows.  A lookup costs two dependent memory accesses whatever
 * the number of rows.  Limits: at most 2^32 - 2 rows (more: DSKGPU_E_STATE, the text says so); an index that does not fit in the
 * free HBM: DSKGPU_E_NOMEM, and the context and its result stay usable.
 * All three run on the context's stream and are synchronous on return.  Like dskgpu_k_*, they do not wait for other streams:
 * bytes that another stream is still writing into d_kmers / d_bytes must be ordered by the caller.  A query changes nothing else in
 * the context: the reads (a kept encoding of dskgpu_encode_reads included), the result, the stats and the sender state stay as they
 * are -- count, query another stream, count again gives identical rows.
 * Errors: no result DSKGPU_E_STATE; n / nbytes == 0: DSKGPU_OK, nothing is done; a null pointer DSKGPU_E_ARG.  A result with zero
 * rows answers 0 everywhere. */
/* Build the index now (optional: both calls below build it on first use). */
int dskgpu_query_prepare(dskgpu_ctx* ctx);
/* d_kmers: n k-mer values on the device, each `words` = ceil(k / 32) u64, row-major, least-significant word first -- the layout of
 * dskgpu_partition_copy and dskgpu_k_enumerate.  d_abundance: n u32 on the device; out[i] = abundance of the solid row with that
 * value, 0 when no row has it (a row's abundance is never 0).  A value that is not canonical, or is >= 4^k, is simply not found. */
int dskgpu_query_kmers(dskgpu_ctx* ctx, const void* d_kmers, uint64_t n, void* d_abundance);
/* d_bytes: a read stream on the device (the input convention above; any alignment).  d_abundance: nbytes u32 on the device; out[p] =
 * abundance of the canonical k-mer of the window ending at byte p when that window is valid and the k-mer is a solid row, else 0.
 * Positions and validity are exactly those of dskgpu_k_enumerate. */
int dskgpu_query_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_abundance);

/* ---- the rows' de Bruijn neighbours: DSK's output is the node set of a de Bruijn graph, and what gatb-core's consumers (the `Graph`
 * built from the solid k-mers, Minia, BCALM, Bloocoo) ask every node first is which of its four successors and four predecessors are
 * solid too -- branching nodes, tips, isolated nodes and unitig ends all follow from that one byte per node.
 * For a k-mer value x < 4^k read as the string s[0..k-1] (A=0 C=1 T=2 G=3, first base most significant):
 *   succ_b(x) = s[1..k-1].b = ((x << 2) | b) & (4^k - 1)        pred_b(x) = b.s[0..k-2] = (x >> 2) | (b << 2(k-1))
 * adj(x) is one byte: bit b (b = 0..3) is set iff canonical(succ_b(x)) is a row of the current result, bit 4 + b iff canonical(pred_b(x))
 * is one -- "row" exactly as dskgpu_query_kmers means it, for every k (1..128) and every result a context can hold (either row order,
 * DSKGPU_F_NO_SORT, several passes, the per-bank modes, a rank's rows).  Nothing is special-cased: a self-loop (poly-A: succ_A(x) = x) sets
 * its bit because x is a row; a palindrome (even k) has successor and predecessor bits that name the same canonical neighbour.  For a row,
 * x is the row's (canonical) value; in- and out-degree in that orientation are the popcounts of the high and the low nibble.
 * A rank's rows are the k-mers that rank owns and every k-mer has one owner, so the adjacency of a GROUP's rows is the bitwise OR over the
 * ranks of dskgpu_graph_neighbors, asked with the same values on every rank's context (dskgpu_group_ctx(g, r)); there is no routed group
 * call.
 * Both calls probe the lookup index above (built on first use, dropped with the result; its limit of 2^32 - 2 rows and its
 * DSKGPU_E_NOMEM hold here too), run on the context's stream, are synchronous on return and change nothing else in the context: the
 * reads (a kept encoding included), the result, the stats and the sender state stay as they are.  Stage time: "graph" (and "query index"
 * when the call built the index).
 * Errors: no result DSKGPU_E_STATE; a null ctx DSKGPU_E_ARG; dskgpu_graph_neighbors with n == 0: DSKGPU_OK, nothing is done; a null
 * d_kmers / d_adj with n > 0, or d_adj and degrees both null: DSKGPU_E_ARG.  A result with zero rows: dskgpu_graph_adjacency writes
 * nothing to d_adj and zero-fills degrees; dskgpu_graph_neighbors answers 0 everywhere. */
/* d_adj: n_rows bytes on the device (dskgpu_result_device's n_rows, result order), may be NULL;
 * degrees: 25 uint64 on the HOST, degrees[i * 5 + o] = rows with i predecessors and o successors, may be NULL; not both NULL. */
int dskgpu_graph_adjacency(dskgpu_ctx* ctx, void* d_adj, uint64_t* degrees);
/* adj() of n caller-supplied values (layout of dskgpu_query_kmers: `words` u64 each, LSW first), canonical or not,
 * whether or not the value itself is a row; a value >= 4^k answers 0.  d_adj: n bytes on the device. */
int dskgpu_graph_neighbors(dskgpu_ctx* ctx, const void* d_kmers, uint64_t n, void* d_adj);

/* ---- the rows' de Bruijn graph compacted into unitigs: what Minia, BCALM and gatb-core's `Graph` do with the node set next -- every
 * maximal non-branching path of solid k-mers becomes one sequence.  On the device, for every k (1..128) and every result a context of
 * world_size 1 can hold (either row order, DSKGPU_F_NO_SORT, several passes, the per-bank modes).
 * Row r (a row number of dskgpu_result_device) with the canonical string S(r) gives two ORIENTED nodes o = 2 r + s: str(o) = S(r) for
 * s = 0, its reverse complement for s = 1; flip(o) = o ^ 1.  succ(o) = the oriented nodes p with str(p) = str(o)[1..] . b for a base b
 * and row(p) a row; outdeg(o) = the popcount of the low (s = 0) or high (s = 1) nibble of the row's adjacency byte above;
 * indeg(p) = outdeg(flip(p)).  LINK: next(o) = p when outdeg(o) = 1 and p is that successor, indeg(p) = 1, row(p) != row(o) (no
 * self-loop such as poly-A, no hairpin such as the AT repeat at odd k) and neither row is its own reverse complement (a palindrome, even k
 * only, is a unitig by itself).  Links are symmetric: next(o) = p <=> next(flip(p)) = flip(o).
 * A UNITIG is a maximal path o_0 -> .. -> o_{L-1} of links; every row lies in exactly one, at one position, in one orientation:
 *   chain        no link into o_0, none out of o_{L-1}, L >= 2: of its two readings the one with row(o_0) < row(o_{L-1});
 *   single node  L = 1, reported forward (s = 0);
 *   cycle        every node has a link into it: starts at the smallest row number on it, forward (o_0 = 2 r_min).
 * Unitigs are numbered 0 .. n_unitigs - 1 by ascending row(o_0).  The sequence of a unitig is str(o_0) followed by the last base of
 * every further str(o_i): k + L - 1 letters of "ACTG".  The unitig STREAM is these sequences, each followed by '\n' -- a read stream by
 * the input convention above: offsets[u] = (rows in unitigs before u) + u * k, stream_bytes = n_rows + n_unitigs * k, and counting
 * the stream with abundance_min = 1 gives back exactly the rows, each once.  The row order changes the numbering, the orientation
 * and where a cycle is cut, never the set of unitigs.
 * The compaction is kept in the context like the lookup index (8 bytes per row + 17 per unitig; about 45 bytes per row more while it
 * is built): built on first use by any of the four calls, dropped when the next count starts and by dskgpu_destroy.  All four probe
 * the lookup index (its DSKGPU_E_NOMEM holds here too, and the context and its result stay usable), run on the context's stream, are
 * synchronous on return and change nothing else in the context: the reads (a kept encoding included), the result, the stats and the sender
 * state stay as they are.  The build ranks the nodes of every path by pointer jumping: at most 33 rounds per phase by construction
 * (2^33 > 2 * rows); a phase that has not finished by then is DSKGPU_E_DEVICE.  Stage times: "unitigs" (the build), "unitig stream", and
 * "graph" / "query index" when the call computed the adjacency / built the index.
 * Errors: a null ctx DSKGPU_E_ARG; no result DSKGPU_E_STATE; more than 2^31 - 1 rows DSKGPU_E_STATE (oriented node numbers are 32 bits;
 * the text says so); a context with world_size > 1 DSKGPU_E_STATE: a rank holds only the k-mers it owns, and the unitigs of a rank's rows
 * do NOT combine into the group's unitigs the way the adjacency bytes OR -- a path ends wherever its next k-mer has another owner.  A
 * result with zero rows: all-zero stats, offsets[0] = 0, nothing else is written. */
typedef struct dskgpu_unitig_stats {
    uint64_t n_unitigs, n_cycles, n_single, max_nodes, stream_bytes, n_rounds, reserved[2];
} dskgpu_unitig_stats;                                   /* 64 bytes */
/* Build the compaction now (optional) and fill `stats` (may be NULL): unitigs, those that are cycles, those of one node, rows of the
 * longest, bytes of the stream, pointer-jumping launches of the build (all phases together). */
int dskgpu_unitigs(dskgpu_ctx* ctx, dskgpu_unitig_stats* stats);
/* Per row, on the device, result order: d_unitig u32[n_rows] = the row's unitig, d_pos u32[n_rows] = (position in it << 1) | s.
 * Either may be NULL; both NULL: DSKGPU_E_ARG. */
int dskgpu_unitigs_rows(dskgpu_ctx* ctx, void* d_unitig, void* d_pos);
/* Per unitig, on the device: d_offsets u64[n_unitigs + 1] byte offsets into the stream, d_ab_sum u64[n_unitigs] sum of the member rows'
 * abundances (BCALM's km, kept exact), d_kind u8[n_unitigs] 0 = chain or single node, 1 = cycle.  Any may be NULL; all NULL: DSKGPU_E_ARG. */
int dskgpu_unitigs_table(dskgpu_ctx* ctx, void* d_offsets, void* d_ab_sum, void* d_kind);
/* The unitig stream into d_bytes (device, any alignment).  capacity < stream_bytes, or a null d_bytes: DSKGPU_E_ARG, nothing is written. */
int dskgpu_unitigs_stream(dskgpu_ctx* ctx, void* d_bytes, uint64_t capacity);

/* ---- unitig links: the EDGES of the compacted de Bruijn graph -- what BCALM writes on every FASTA header (L:+:17:-) and GFA on its L
 * lines, and where tip clipping, bubble popping and every traversal start: "what hangs on this end of this unitig".
 * An ORIENTED UNITIG is U = 2 u + t: t = 0 reads unitig u as dskgpu_unitigs_stream gives it, t = 1 reads its reverse complement;
 * flip(U) = U ^ 1.  With the path o_0 .. o_{L-1} of unitig u (above): first(2u) = o_0, last(2u) = o_{L-1}, first(2u + 1) = flip(o_{L-1}),
 * last(2u + 1) = flip(o_0).  EDGE U -> V <=> first(V) is in succ(last(U)), succ on oriented nodes as above.  A row that is its own reverse
 * complement is named only by its forward node 2 r (as its adjacency bits are), so an edge into a palindrome's unitig v always has V = 2 v.
 * What follows from the definition of the links:
 *   - every successor of last(U) is first(V) for exactly one V: no edge ever lands inside a unitig (the build checks it; a violation is
 *     DSKGPU_E_DEVICE, an internal error);
 *   - the targets of one U are distinct and at most 4, so there are at most 8 * n_unitigs edges;
 *   - a cycle has exactly the edges 2u -> 2u and 2u + 1 -> 2u + 1: the link that closes it;
 *   - outside the unitigs of palindromes, U -> V <=> flip(V) -> flip(U).
 * The edges of U are ordered by the base appended to str(last(U)), in the order A, C, T, G.  The sequences of U and V overlap by k - 1
 * letters (GFA: "<k-1>M").
 * The edges are kept in the context with the compaction (about 12 bytes per oriented unitig + 4 per edge; 24 bytes per oriented unitig
 * more while they are built): built on first use by either call -- which builds the compaction and the lookup index below them when they
 * are not there yet --, dropped when the next count starts and by dskgpu_destroy.  Both calls run on the context's stream, are synchronous
 * on return and change nothing else in the context: the reads (a kept encoding included), the result, the stats and the sender state stay as
 * they are.  Stage time: "unitig edges" (and those of the compaction when the call built it).
 * Errors: a null ctx DSKGPU_E_ARG; no result DSKGPU_E_STATE; more than 2^31 - 1 rows DSKGPU_E_STATE; a context with world_size > 1
 * DSKGPU_E_STATE (the text names world_size): a rank's unitigs are not the group's; the index, the compaction or the edges do not fit
 * DSKGPU_E_NOMEM, and the context, its result and what was built before stay usable.  A result with zero rows: all-zero stats,
 * d_offsets[0] = 0, nothing else is written. */
typedef struct dskgpu_unitig_edge_stats {
    uint64_t n_edges, n_self, n_dead_ends, max_degree, reserved[4];
} dskgpu_unitig_edge_stats;                              /* 64 bytes */
/* Build the edges now (optional) and fill `stats` (may be NULL): edges, those whose two unitigs are the same u, oriented unitigs without
 * an edge, the most edges of one oriented unitig (0..4). */
int dskgpu_unitig_edges(dskgpu_ctx* ctx, dskgpu_unitig_edge_stats* stats);
/* On the device: d_offsets u64[2 * n_unitigs + 1], the edges of U are d_targets[d_offsets[U] .. d_offsets[U + 1]) (CSR;
 * d_offsets[2 * n_unitigs] = n_edges); d_targets u32[n_edges] the oriented unitigs V; d_ends u32[2 * n_unitigs], ends[U] = last(U) as an
 * oriented node number 2 r + s -- the way back from a unitig to its rows.  Any may be NULL; all NULL: DSKGPU_E_ARG. */
int dskgpu_unitig_edges_table(dskgpu_ctx* ctx, void* d_offsets, void* d_targets, void* d_ends);

/* ---- tip clipping: the first call that CHANGES a graph -- what Minia, BCALM's tip removal and gatb-core's `Graph` simplifications do
 * before anything else, because on real reads the compacted graph is dominated by the short dead ends that sequencing errors leave.
 * Two pieces: a way to take rows out of a result (dskgpu_filter_rows), after which every call above serves the graph of the kept rows with
 * the code it has, and the tip rule on the tables of the compaction and the edges (dskgpu_graph_tips; dskgpu_clip_tips runs rounds of both).
 * Everything is exact integer arithmetic; nothing depends on the row order except the numbering.
 * With unitig u of L[u] = (offsets[u + 1] - offsets[u]) - k rows, S[u] = ab_sum[u], kind[u], its readings U = 2u + t, E(U) = the targets of U in
 * the table of dskgpu_unitig_edges_table and deg(U) = |E(U)|:
 *   CANDIDATE  cand[u] <=> kind[u] == 0, L[u] <= max_nodes, exactly one of deg(2u), deg(2u + 1) is 0, and max_abundance == 0 or
 *              S[u] <= max_abundance * L[u].  The ATTACHED END A(u) is the one of 2u, 2u + 1 that has edges.
 *   SIBLINGS   of u: the unitigs w = X >> 1 with X in E(V ^ 1) for some V in E(A(u)), w != u -- what else hangs on the nodes u hangs on;
 *              read off the tables as they are (palindromes need no special case), at most 4 x 4 entries.
 *   STRONGER   stronger(w, u) <=> S[w] * L[u] > S[u] * L[w], or the products are equal and L[w] > L[u] (max_nodes <= 65535 keeps the
 *              products of two candidates inside 64 bits).
 *   TIP        tip[u] <=> cand[u] and some sibling w has !cand[w] or stronger(w, u); OUTRANKED when no sibling has !cand[w], so that only
 *              stronger candidates clipped it.
 * So a dead start that forks is never clipped (it has no sibling), two equally strong short ends of a fork both stay, and an isolated
 * unitig is never clipped.  A ROUND removes the rows of all tips; the graph of the remaining rows is compacted again, and a round that
 * finds no tip ends the loop.  Bubbles are popped by the calls of the next section, and a rank of a group (world_size > 1) has no
 * compaction to clip. */
typedef struct dskgpu_tip_params {
    uint32_t max_nodes, max_abundance, max_rounds, reserved[5];
} dskgpu_tip_params;                                     /* 32 bytes; max_nodes 1..65535, max_abundance 0 = no limit, max_rounds: dskgpu_clip_tips only */
typedef struct dskgpu_tip_stats {
    uint64_t n_candidates, n_tips, n_outranked, n_rows_clipped, n_rounds, n_rows_left, reserved[2];
} dskgpu_tip_stats;                                      /* 64 bytes */
/* Keep the rows r of the current result with d_keep[r] != 0 (d_keep: n_rows bytes on the device, result order) and drop the others.
 * The kept rows stay in their order, word arrays and abundance; dskgpu_result_device and every partition accessor describe them from now
 * on.  The number of partitions is unchanged: in the global order (and with DSKGPU_F_NO_SORT) they are the usual n * p / P ranges of the new
 * n_rows; with DSKGPU_F_PARTITION_ORDER partition p holds exactly the kept rows of the old partition p -- one pass or several --, still ascending.
 * For every k and every result a context can hold, a rank's rows (world_size > 1) included.
 * The lookup index, the compaction and the edges are dropped: the next call that needs them builds them over the kept rows.
 * dskgpu_get_stats and dskgpu_histogram stay the COUNT's record -- n_solid is what the count found, not what is left; the rows left are
 * dskgpu_result_device's n_rows.  The reads, a kept encoding and the sender state are untouched.  The kept rows live in buffers of the
 * context's own (a second filter reads one set and writes another), freed, with the scratch of these calls (9 bytes per row), when the next count starts and by dskgpu_destroy; when they do
 * not fit: DSKGPU_E_NOMEM and the result is unchanged.  *n_kept (may be NULL) = the rows left.  Runs on the context's stream, synchronous
 * on return.  Stage time: "filter rows".
 * Errors: a null ctx, or a null d_keep while there are rows, DSKGPU_E_ARG; no result DSKGPU_E_STATE.  A result with zero rows: DSKGPU_OK,
 * n_kept = 0, nothing is done. */
int dskgpu_filter_rows(dskgpu_ctx* ctx, const void* d_keep, uint64_t* n_kept);
/* One round of the rule on the current result; no row changes.  d_row_tip u8[n_rows]: 1 = the row's unitig is a tip; d_unitig_tip
 * u8[n_unitigs]: bit 0 = candidate, bit 1 = tip, bit 2 = outranked; stats: the counts of this round with n_rounds = 1 and n_rows_left =
 * n_rows - n_rows_clipped.  Any may be NULL; all three NULL: DSKGPU_E_ARG.  Builds the edges (and the compaction and the index below them)
 * when they are not there, and changes nothing else in the context: the reads (a kept encoding included), the result, the stats and the
 * sender state stay as they are.  Stage time: "tips" (and those of what the call built).
 * Errors: a null ctx or params, max_nodes 0 or > 65535: DSKGPU_E_ARG; no result DSKGPU_E_STATE; a context with world_size > 1
 * DSKGPU_E_STATE (the text names world_size); the limits and DSKGPU_E_NOMEM of dskgpu_unitig_edges.  A result with zero rows: all-zero
 * stats, nothing is written. */
int dskgpu_graph_tips(dskgpu_ctx* ctx, const dskgpu_tip_params* params, void* d_row_tip, void* d_unitig_tip, dskgpu_tip_stats* stats);
/* Rounds of (dskgpu_graph_tips -> dskgpu_filter_rows of the rows that are on no tip) until a round finds no tip or max_rounds rounds
 * have clipped (1..64; 0 = 64; more: DSKGPU_E_ARG).  stats (may be NULL): the sums over the rounds that ran, the last one that found no
 * tip included -- a stop by max_rounds evaluates no further round, so n_candidates then holds the clipping rounds only --; n_rounds = the rounds that clipped something, n_rows_left = the final n_rows.  On return the compaction and the edges of
 * the FINAL rows are built: dskgpu_unitigs_stream, dskgpu_unitig_edges_table (and a GFA written from them) give the cleaned graph at once.
 * What dskgpu_filter_rows says about the rest of the context holds here.  A round reads back one small record; an error in a later round
 * (DSKGPU_E_NOMEM, say) leaves the result of the rounds already done, which is a consistent result like any other, and stats says
 * how far the call came.  Stage times: "tips", "filter rows", and "query index" / "graph" / "unitigs" / "unitig edges" of every rebuild.
 * Errors: those of dskgpu_graph_tips. */
int dskgpu_clip_tips(dskgpu_ctx* ctx, const dskgpu_tip_params* params, dskgpu_tip_stats* stats);

/* ---- bubble popping: the other half of what an assembler does before it reads a contig off the graph.  Tips are the errors near a read's
 * end; bubbles are the errors, and the SNPs, in its middle: two or more parallel unitigs between the same two ends, one of them weak.
 * The rule reads the same tables as the tip rule and a round takes rows out the same way (dskgpu_filter_rows); exact integer arithmetic,
 * nothing depends on the row order except the numbering.  In the notation of the tip section:
 *   CANDIDATE  cand[u] <=> kind[u] == 0, L[u] <= max_nodes, deg(2u) == 1 and deg(2u + 1) == 1, and with out(u) = E(2u)[0] and in(u) =
 *              E(2u + 1)[0] neither out(u) >> 1 nor in(u) >> 1 is u.  So u is a simple path from P = in(u) ^ 1 to out(u).
 *   SIBLINGS   of a candidate u: the unitigs w = X >> 1 for X in E(in(u) ^ 1) (at most 4) with w != u, cand[w], E(X)[0] == out(u),
 *              E(X ^ 1)[0] == in(u) and |L[w] - L[u]| <= max_diff -- the same two ends, read in the orientation in which P reaches w
 *              (X even: out(w) == out(u) and in(w) == in(u); X odd: in(w) == out(u) and out(w) == in(u)).  The tables are read as they
 *              are; palindromes get no special case.
 *   STRONGER   as for tips: S[w] * L[u] > S[u] * L[w], or the products are equal and L[w] > L[u].
 *   POPPED     pop[u] <=> cand[u] and some sibling is stronger than u.  IN A BUBBLE <=> cand[u] and u has at least one sibling.
 * So equally strong branches all stay, of a three-way bubble the two weaker go in one round, and a unitig with more than one edge at an
 * end is never popped.  A ROUND removes the rows of all popped unitigs; the graph of the remaining rows is compacted again, and a round
 * that pops nothing ends the loop.  A dead-end branch that carries a bubble is no tip before the bubble is popped, and a popped bubble can
 * leave a new tip: dskgpu_simplify runs both in turn until the graph stops changing. */
typedef struct dskgpu_bubble_params {
    uint32_t max_nodes, max_diff, max_rounds, reserved[5];
} dskgpu_bubble_params;                                  /* 32 bytes; max_nodes 1..65535, max_diff 0 = equal lengths only, max_rounds: dskgpu_pop_bubbles / dskgpu_simplify only */
typedef struct dskgpu_bubble_stats {
    uint64_t n_candidates, n_in_bubbles, n_popped, n_rows_popped, n_rounds, n_rows_left, reserved[2];
} dskgpu_bubble_stats;                                   /* 64 bytes */
typedef struct dskgpu_simplify_stats {
    uint64_t n_passes, n_rows_left, reserved[6];
    dskgpu_tip_stats tips;
    dskgpu_bubble_stats bubbles;
} dskgpu_simplify_stats;                                 /* 192 bytes */
/* One round of the rule on the current result; no row changes.  d_row_pop u8[n_rows]: 1 = the row's unitig is popped; d_unitig_bits
 * u8[n_unitigs]: bit 0 = candidate, bit 1 = popped, bit 2 = in a bubble; stats: the counts of this round with n_rounds = 1 and
 * n_rows_left = n_rows - n_rows_popped.  The outputs, their NULL rules, what the call builds, what it leaves alone and its errors are
 * those of dskgpu_graph_tips.  Stage time: "bubbles" (and those of what the call built). */
int dskgpu_graph_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, void* d_row_pop, void* d_unitig_bits, dskgpu_bubble_stats* stats);
/* Rounds of (dskgpu_graph_bubbles -> dskgpu_filter_rows of the rows that are on no popped unitig) until a round pops nothing or max_rounds
 * rounds have popped (1..64; 0 = 64; more: DSKGPU_E_ARG), with the contract of dskgpu_clip_tips: stats (may be NULL) holds the sums over the
 * rounds that ran, n_rounds = the rounds that popped something, n_rows_left = the final n_rows; a round reads back one small record; an
 * error in a later round leaves the consistent result of the rounds already done; on return the compaction and the edges of the FINAL rows
 * are built.  Stage times: "bubbles", "filter rows", and those of every rebuild.  Errors: those of dskgpu_graph_tips. */
int dskgpu_pop_bubbles(dskgpu_ctx* ctx, const dskgpu_bubble_params* params, dskgpu_bubble_stats* stats);
/* Passes of (dskgpu_clip_tips, then dskgpu_pop_bubbles) until a pass removes no row or max_passes passes have run (1..16; 0 = 16; more:
 * DSKGPU_E_ARG).  A NULL tip_params or bubble_params skips that half; both NULL: DSKGPU_E_ARG.  stats (may be NULL): n_passes = the passes
 * that removed a row, tips / bubbles = the sums of the two calls' stats over the passes that ran (n_rounds summed too), n_rows_left = the
 * final n_rows, in all three places.  An error ends the call with the result of what was done, as for dskgpu_clip_tips.
 * Errors: those of the two calls, checked for both sets of parameters before anything runs. */
int dskgpu_simplify(dskgpu_ctx* ctx, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params, uint32_t max_passes, dskgpu_simplify_stats* stats);

/* ---- erroneous connections: the third of the simplifications that Minia and gatb-core's `Graph` run, after tips and bulges.  An erroneous
 * connection is a short, weakly covered unitig attached at BOTH ends, bridging two well-covered places -- what a chimeric read leaves, a
 * sequencing error inside a repeat, or a weak branch whose ends fork.  The tip rule ignores it (no dead end), the bubble rule ignores it
 * unless both ends have exactly one edge and a parallel chain runs between the same two ends; it joins components that should be separate
 * and splits contigs at forks that should not be there.  The rule reads the same tables as the tip rule and a round takes rows out the same
 * way (dskgpu_filter_rows); exact integer arithmetic, nothing depends on the row order except the numbering.  In the notation of the tip
 * section:
 *   CANDIDATE  cand[u] <=> kind[u] == 0, L[u] <= max_nodes, deg(2u) >= 1 and deg(2u + 1) >= 1, no target of either end is a reading of u
 *              (V >> 1 != u for every V in E(2u) and E(2u + 1)), and max_abundance == 0 or S[u] <= max_abundance * L[u].
 *   FLANK      of an end A (2u or 2u + 1): the unitigs V >> 1 for V in E(A), together with X >> 1 for X in E(V ^ 1) for those V, without u
 *              itself -- everything that meets u's end at that junction: what u runs into, and what else runs into the same nodes.  At
 *              most 4 + 16 entries; the tables are read as they are, palindromes get no special case.
 *   WEAK AT A  weak(A) <=> some w in FLANK(A) has S[w] * L[u] > min_ratio * S[u] * L[w] (strict): the mean abundance of w is more than
 *              min_ratio times that of u.  The products reach 2^87 and are compared in 128 bits.
 *   REMOVED    rem[u] <=> cand[u], weak(2u) and weak(2u + 1).  ONE-SIDED <=> cand[u] and exactly one end is weak.
 * min_ratio >= 2 has two consequences: two unitigs can never each be the reason the other is removed, and every removed unitig has, at
 * each end, a flank unitig that stays in that round.  A ROUND removes the rows of all removed unitigs; the graph of the remaining rows is
 * compacted again, and a round that removes nothing ends the loop.  dskgpu_simplify_all runs the three rules in turn. */
typedef struct dskgpu_connection_params {
    uint32_t max_nodes, min_ratio, max_abundance, max_rounds, reserved[4];
} dskgpu_connection_params;                              /* 32 bytes; max_nodes 1..65535, min_ratio 2..255, max_abundance 0 = no limit, max_rounds: dskgpu_remove_connections / dskgpu_simplify_all only */
typedef struct dskgpu_connection_stats {
    uint64_t n_candidates, n_one_sided, n_removed, n_rows_removed, n_rounds, n_rows_left, reserved[2];
} dskgpu_connection_stats;                               /* 64 bytes */
typedef struct dskgpu_simplify_all_stats {
    uint64_t n_passes, n_rows_left, reserved[6];
    dskgpu_tip_stats tips;
    dskgpu_bubble_stats bubbles;
    dskgpu_connection_stats connections;
} dskgpu_simplify_all_stats;                             /* 256 bytes */
/* One round of the rule on the current result; no row changes.  d_row_rem u8[n_rows]: 1 = the row's unitig is removed; d_unitig_bits
 * u8[n_unitigs]: bit 0 = candidate, bit 1 = removed, bit 2 = weak at the end 2u, bit 3 = weak at the end 2u + 1; stats: the counts of this
 * round with n_rounds = 1 and n_rows_left = n_rows - n_rows_removed.  The outputs, their NULL rules, what the call builds, what it leaves
 * alone and its errors are those of dskgpu_graph_bubbles; in addition min_ratio < 2 or > 255: DSKGPU_E_ARG.  Stage time: "connections"
 * (and those of what the call built). */
int dskgpu_graph_connections(dskgpu_ctx* ctx, const dskgpu_connection_params* params, void* d_row_rem, void* d_unitig_bits, dskgpu_connection_stats* stats);
/* Rounds of (dskgpu_graph_connections -> dskgpu_filter_rows of the rows that are on no removed unitig) until a round removes nothing or
 * max_rounds rounds have removed (1..64; 0 = 64; more: DSKGPU_E_ARG), with the contract of dskgpu_pop_bubbles: stats (may be NULL) holds
 * the sums over the rounds that ran, n_rounds = the rounds that removed something, n_rows_left = the final n_rows; a round reads back one
 * small record; an error in a later round leaves the consistent result of the rounds already done; on return the compaction and the edges
 * of the FINAL rows are built.  Stage times: "connections", "filter rows", and those of every rebuild.  Errors: those of
 * dskgpu_graph_connections. */
int dskgpu_remove_connections(dskgpu_ctx* ctx, const dskgpu_connection_params* params, dskgpu_connection_stats* stats);
/* Passes of (dskgpu_clip_tips, then dskgpu_pop_bubbles, then dskgpu_remove_connections) until a pass removes no row or max_passes passes
 * have run (1..16; 0 = 16; more: DSKGPU_E_ARG).  A NULL parameter set skips that part; all three NULL: DSKGPU_E_ARG.  With
 * connection_params == NULL the rows left and the tips / bubbles stats are exactly those of dskgpu_simplify.  stats (may be NULL): as for
 * dskgpu_simplify, with the sums of the third call in connections and n_rows_left = the final n_rows in all four places.
 * Errors: those of the three calls, checked for all sets of parameters before anything runs. */
int dskgpu_simplify_all(dskgpu_ctx* ctx, const dskgpu_tip_params* tip_params, const dskgpu_bubble_params* bubble_params,
                        const dskgpu_connection_params* connection_params, uint32_t max_passes, dskgpu_simplify_all_stats* stats);

/* ---- connected components: the first GLOBAL question about the graph -- which pieces does it fall into, and how big is each?  Every call
 * above looks at one unitig and its neighbours.  Clipping and popping leave small isolated pieces behind -- chains of error k-mers that hang on
 * nothing, short contaminant fragments: neither tips (an isolated unitig is never clipped) nor bubbles --, which every assembler removes by
 * size right after tips and bubbles; and a metagenome or transcriptome graph is processed, drawn and binned piece by piece, from one
 * component label per unitig.  Exact integer arithmetic; in the notation of the unitig, edge and tip sections (unitig u, readings U = 2u + t,
 * E(U), L[u], S[u] = ab_sum[u]):
 *   JOINED     u ~ v <=> some entry of the CSR table of dskgpu_unitig_edges_table has source U and target V with U >> 1 == u and V >> 1 == v.
 *              Every entry counts in both directions; self edges join nothing.
 *   SYMMETRY   for every entry U -> V there is an entry from a reading of v to a reading of u: outside the unitigs of palindromes this is
 *              the last fact of the edge section (flip(V) -> flip(U)); for an edge into a palindrome's unitig 2v, both readings of v have
 *              the successors of the one node, and one of them is first(U ^ 1).  The device treats every entry as undirected and does not
 *              need it.
 *   COMPONENT  a class of the reflexive-transitive closure of ~; its LABEL is the smallest unitig number in it.  Components are numbered
 *              0 .. n_components - 1 by ascending label, first[c].  A cycle unitig with no other edge, a palindrome without neighbours and
 *              every other isolated unitig is a component by itself.
 *   TABLE      per component c: unitigs[c] = its unitigs, rows[c] = the sum of their L[u], ab_sum[c] = the sum of their S[u] (exact in 64
 *              bits), edges[c] = the CSR entries whose source lies in c, self edges included.  The columns add up to n_unitigs, n_rows, the
 *              sum of all abundances and n_edges.  The bases of a component are rows[c] + (k - 1) * unitigs[c].
 *   SMALL      small[c] <=> rows[c] < min_rows && (max_abundance == 0 || ab_sum[c] <= (uint64_t)max_abundance * rows[c]).  min_rows counts
 *              k-mers and is at least 1; rows[c] < 2^31, so the product stays inside 64 bits.
 * The row order changes the numbering, never the partition of the k-mers; nothing depends on it otherwise.
 * ONE APPLICATION IS FINAL: removing whole components changes no adjacency byte of any kept row, so the unitigs, the edges and the
 * components of the kept rows are exactly the old ones that were not small, renumbered; a second application removes nothing; there are no
 * rounds.
 * The labelling is a lock-free union-find that hooks the larger root under the smaller, so the labels do not depend on scheduling, and it is
 * three launches whatever the graph (set the parents, hook, flatten): there is no round count to bound, n_rounds is always 3 (0 for a result
 * without rows).  A walk that does not end within 4 * n_unitigs + 64 steps -- none can -- is DSKGPU_E_DEVICE, an internal error.
 * The components are kept in the context with the edges (4 bytes per unitig + 36 per component; 12 bytes per unitig more, and the scan's
 * scratch, while they are built): built on first use by any of the five calls -- which build the edges, the compaction and the lookup index
 * below them when they are not there yet --, dropped or invalidated wherever the edges are: when the next count starts, by
 * dskgpu_filter_rows (and so by dskgpu_clip_tips / _pop_bubbles / _simplify) and by dskgpu_destroy.  The calls run on the context's stream, are
 * synchronous on return and change nothing else in the context: the reads (a kept encoding included), the result, the stats and the sender
 * state stay as they are.  Stage times: "components" (the build), "component rows" (d_row_comp), "small components", "filter rows", and
 * those of what a call built below them.
 * Errors: a null ctx DSKGPU_E_ARG; no result DSKGPU_E_STATE; more than 2^31 - 1 rows DSKGPU_E_STATE; a context with world_size > 1
 * DSKGPU_E_STATE (the text names world_size): a rank's unitigs are not the group's; DSKGPU_E_NOMEM leaves the context, its result and what
 * was built before usable.  A result with zero rows: all-zero stats, nothing is written. */
typedef struct dskgpu_component_stats {
    uint64_t n_components, n_single, max_unitigs, max_rows, n_rounds, reserved[3];
} dskgpu_component_stats;                                /* 64 bytes; n_single: components of one unitig; max_*: the most unitigs / rows of one component; n_rounds: launches of the labelling */
typedef struct dskgpu_component_params {
    uint32_t min_rows, max_abundance, reserved[6];
} dskgpu_component_params;                               /* 32 bytes; min_rows >= 1, max_abundance 0 = no limit */
typedef struct dskgpu_component_drop_stats {
    uint64_t n_small, n_unitigs_dropped, n_rows_dropped, n_rows_left, reserved[4];
} dskgpu_component_drop_stats;                           /* 64 bytes */
/* Build the components now (optional) and fill `stats` (may be NULL). */
int dskgpu_components(dskgpu_ctx* ctx, dskgpu_component_stats* stats);
/* On the device: d_unitig_comp u32[n_unitigs] = the component of every unitig, d_row_comp u32[n_rows] = that of every row's unitig (result
 * order).  Either may be NULL; both NULL: DSKGPU_E_ARG. */
int dskgpu_components_labels(dskgpu_ctx* ctx, void* d_unitig_comp, void* d_row_comp);
/* The table, on the device: d_first u32[n_components], the four columns u64[n_components] each.  Any may be NULL; all NULL: DSKGPU_E_ARG. */
int dskgpu_components_table(dskgpu_ctx* ctx, void* d_first, void* d_unitigs, void* d_rows, void* d_ab_sum, void* d_edges);
/* The rule on the current result; no row changes.  d_row_drop u8[n_rows]: 1 = the row's component is small; d_comp_small u8[n_components]:
 * 1 = small; stats: the small components, their unitigs and rows, n_rows_left = n_rows - n_rows_dropped.  Any may be NULL; all three NULL, a
 * NULL params or min_rows == 0: DSKGPU_E_ARG. */
int dskgpu_graph_small_components(dskgpu_ctx* ctx, const dskgpu_component_params* params, void* d_row_drop, void* d_comp_small, dskgpu_component_drop_stats* stats);
/* Mark the small components, take their rows out with one dskgpu_filter_rows and leave the compaction, the edges and the components of the
 * FINAL rows built, like dskgpu_clip_tips.  When nothing is small nothing is filtered and nothing invalidated.  What dskgpu_filter_rows says
 * about the count's stats, the histogram, the partitions of either row order and a kept threading holds here.  stats (may be NULL): what was
 * dropped, n_rows_left = the final n_rows.  Errors: those of dskgpu_graph_small_components. */
int dskgpu_drop_components(dskgpu_ctx* ctx, const dskgpu_component_params* params, dskgpu_component_drop_stats* stats);

/* ---- reads threaded through the compacted graph: the way back from reads to the graph that the calls above build and clean -- what
 * Minia's contig stage, the users of BCALM / Bandage and every repeat resolution ask next: where on the graph does this read lie, and which
 * edges does it walk?  A count at k gives the abundance of the nodes; an edge U -> V is a (k+1)-mer, so its read support needs the reads.
 * In the notation of the unitig and edge sections (row r, oriented node o = 2 r + s, oriented unitig U = 2 u + t, first(U), last(U), E(U),
 * L[u] = the rows of u) and with text(U) = the sequence of u as dskgpu_unitigs_stream gives it for t = 0, its reverse complement for t = 1:
 *   PLACEMENT  of byte position p of a read stream (the input convention above, any alignment): the window ending at p is PLACED when it is
 *              valid (exactly dskgpu_k_enumerate's validity) and its canonical k-mer is a row r of the current result.  Its node is
 *              o(p) = 2 r + s, s = 0 when the window read forward equals the canonical string (a row that is its own reverse complement:
 *              always s = 0), else s = 1.  With unitig[r] = u and pos[r] = (i << 1) | s_r (dskgpu_unitigs_rows): U(p) = 2 u, j(p) = i when
 *              s == s_r, else U(p) = 2 u + 1, j(p) = L[u] - 1 - i; a palindromic row has U(p) = 2 u, j(p) = 0.  Equivalently:
 *              text(U(p))[j(p) .. j(p) + k) is the window in upper case, and of the two readings of a palindrome's unitig the even one is
 *              named.  Not placed: U = 0xFFFFFFFF, j = 0.
 *   WALK       a maximal run of consecutive placed positions first .. last: it never crosses a byte that ends a window, nor a k-mer that is
 *              no row.  Inside a walk, position p > first is an EDGE STEP when j(p) == 0, else an INSIDE STEP.  From the link rules: an inside
 *              step has U(p) = U(p - 1) and j(p) = j(p - 1) + 1; an edge step has j(p - 1) = L[U(p - 1) >> 1] - 1 and U(p) in E(U(p - 1)) --
 *              also at the closing edge 2u -> 2u of a cycle, the self edge of poly-A, the hairpin U -> U ^ 1 at odd k, and into and out of a
 *              palindrome's unitig through its even reading.  The device checks that U(p) is among the at most 4 targets of U(p - 1); a miss
 *              is DSKGPU_E_DEVICE, an internal error, as the edge build does for its own fact.
 *   STEPS      of a walk: U(first) followed by U(p) of every edge step, in order.  Its windows number last - first + 1 =
 *              sum of L[U_i >> 1] - j(first) - (L[U_m >> 1] - 1 - j(last)); the steps' texts glued with k - 1 letters of overlap, j(first)
 *              letters cut at the front and L - 1 - j(last) at the back, are the stream's bytes first - k + 1 .. last in upper case.  This
 *              is what GFA calls a path.
 *   SUPPORT    unitig_support[u] = placed positions with U(p) >> 1 == u; edge_support[e] = edge steps whose (U(p - 1), U(p)) is entry e of
 *              the CSR table of dskgpu_unitig_edges_table.
 * Both builders (dskgpu_thread_place, dskgpu_thread_reads) build the edges, the compaction and the lookup index when they are not there,
 * run on the context's stream, are synchronous on return and leave the reads (a kept encoding included), the result, the stats and the
 * sender state alone.  Positions, walks and steps are 64-bit counts; there is no cap on nbytes.  Stage times: "thread place" and "thread
 * walks", plus those of what the call built.
 * Memory: dskgpu_thread_reads takes, and frees before it returns, the 2-bit form of the stream (0.375 bytes per stream byte) + 8 bytes per
 * stream byte for the placements (+ 48 bytes per 1024 stream bytes of block sums); what it keeps is 32 bytes per walk, 4 per step, 8 per
 * unitig and 8 per edge.  A stream too big for the free HBM can be threaded in pieces cut behind any byte that ends a window (a '\n'):
 * walks never cross one, so the pieces' walks concatenate -- first / last shifted by the bytes before the piece -- and the supports add.
 * Errors: a null ctx, a null d_bytes with nbytes > 0: DSKGPU_E_ARG; no result DSKGPU_E_STATE; a context with world_size > 1 DSKGPU_E_STATE
 * and more than 2^31 - 1 rows DSKGPU_E_STATE (the text says so, as for the unitigs); a table call when no threading is kept DSKGPU_E_STATE;
 * DSKGPU_E_NOMEM leaves the context, its result and what was built before usable.  nbytes == 0: DSKGPU_OK, nothing is done, all-zero
 * stats, and the table calls after it write d_offsets[0] = 0 only.  A result with zero rows places nothing: n_valid is still counted,
 * there are no walks. */
typedef struct dskgpu_thread_stats {
    uint64_t n_valid, n_placed, n_walks, n_steps, max_steps, reserved[3];
} dskgpu_thread_stats;                                   /* 64 bytes; valid windows, placed positions, walks, steps, the most steps of one walk */
/* Stateless, like dskgpu_query_reads: d_unitig u32[nbytes] = U(p), d_off u32[nbytes] = j(p), on the device.  Either may be NULL; both NULL:
 * DSKGPU_E_ARG. */
int dskgpu_thread_place(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_unitig, void* d_off);
/* Thread the stream and keep the walks, the steps, both supports and the stats in the context, as the compaction is kept: dropped by the
 * next count, by dskgpu_filter_rows (and so by dskgpu_clip_tips / _pop_bubbles / _simplify), by the next dskgpu_thread_reads and by
 * dskgpu_destroy.  stats may be NULL. */
int dskgpu_thread_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, dskgpu_thread_stats* stats);
/* The kept walks, on the device, numbered by ascending first: d_offsets u64[n_walks + 1] (CSR into the steps; d_offsets[n_walks] = n_steps),
 * d_steps u32[n_steps], d_first / d_last u64[n_walks], d_ends u32[2 * n_walks] = (j(first), j(last)) of every walk.  Any may be NULL; all
 * NULL: DSKGPU_E_ARG. */
int dskgpu_thread_walks(dskgpu_ctx* ctx, void* d_offsets, void* d_steps, void* d_first, void* d_last, void* d_ends);
/* The kept supports, on the device: d_unitig_support u64[n_unitigs], d_edge_support u64[n_edges].  Either may be NULL; both NULL:
 * DSKGPU_E_ARG. */
int dskgpu_thread_support(dskgpu_ctx* ctx, void* d_unitig_support, void* d_edge_support);

/* ---- variant reporting: the bubbles of the compacted graph as pairs of sequences -- what DiscoSnp does on top of a GATB count.  The bubble
 * rule finds every pair of parallel branches between the same two ends; dskgpu_pop_bubbles can only delete the weaker one.  These calls say
 * which unitig is whose sibling, in which reading the two run in parallel, and what differs between them.  They read the tables the bubble
 * rule reads and keep its definitions word for word; exact integer arithmetic, nothing depends on the row order except the numbering.  In
 * the notation of the tip and bubble sections (L[u], S[u], U = 2u + t, E(U), cand, in(u), out(u)) and with text(U) of the threading section,
 * with parameters max_nodes and max_diff:
 *   VARIANT    an unordered pair of unitigs a < b in which b is a SIBLING of a by the bubble rule (siblinghood is symmetric).  Each pair is
 *              reported once, so a three-way bubble gives three variants.
 *   READINGS   from = in(a) ^ 1 and to = out(a); A = 2a; B = the X in E(from) with X >> 1 == b -- the reading in which `from` reaches b,
 *              read off the tables as they are (palindromes get no special case).
 *   ORDER      variants are numbered by ascending (a, b).
 *   DIFFERENCE text(A) and text(B), of na = k + L[a] - 1 and nb = k + L[b] - 1 letters, compared in full: lcp = the length of the longest
 *              common prefix (<= min(na, nb)); lcs = the length of the longest common suffix, capped at min(na, nb) - lcp (the usual
 *              left-aligned trimming; the cap bites for an indel inside a run or tandem repeat).  L[a] == L[b]: n_mismatch = the Hamming
 *              distance, kind = 1 (SNP) when it is 1, kind = 2 (MULTI) when it is 2 or more; it cannot be 0, equal texts would be the
 *              same rows.  L[a] != L[b]: n_mismatch = 0, kind = 3 (INDEL) when lcp + lcs == min(na, nb), else kind = 4 (COMPLEX: a
 *              substitution next to an indel).
 *   RECORD     eight u32 (32 bytes) per variant: A, B, from, to, lcp, lcs, n_mismatch, kind.
 *   STREAM     for variant i: text(A_i) '\n' text(B_i) '\n' -- a read stream by the input convention; offsets u64[2 * n_variants + 1] = the
 *              first byte of every line, the last entry = stream_bytes = sum(L[a] + L[b]) + 2 * n_variants * k.  Counting the stream at k
 *              with abundance_min = 1 gives exactly the rows of the unitigs that are in some variant, each with abundance = the number of
 *              variants its unitig is in.
 * dskgpu_variants finds the variants of the current result, which stays untouched, and keeps the records, the stream and the stats in the
 * context, the way a threading is kept (48 bytes per variant + the stream; while it runs, 33 bytes per unitig, 16 per variant and one byte
 * per letter of the unitigs in a variant -- the whole unitig stream is never made): dropped by the next count, by dskgpu_filter_rows (and so by
 * dskgpu_clip_tips / _pop_bubbles / _simplify / _drop_components), by the next dskgpu_variants and by dskgpu_destroy.  It builds the edges,
 * the compaction and the lookup index when they are not there, and leaves alone the reads (a kept encoding included), the result, the stats,
 * the sender state and a kept threading.  stats (may be NULL): n_unitigs = the unitigs in at least one variant (n_in_bubbles of
 * dskgpu_graph_bubbles with the same parameters), max_letters = the longest text compared.  Runs on the context's stream, synchronous on
 * return.  Stage time: "variants" (and those of what the call built).
 * Errors, as for dskgpu_graph_bubbles: a null ctx or params, max_nodes 0 or > 65535: DSKGPU_E_ARG; no result DSKGPU_E_STATE; a context with
 * world_size > 1 DSKGPU_E_STATE (the text names world_size); more than 2^31 - 1 rows DSKGPU_E_STATE; a copy call when nothing is kept
 * DSKGPU_E_STATE; DSKGPU_E_NOMEM leaves the context, its result and what was built before usable.  A result with zero rows, or zero
 * variants: all-zero stats, and the copy calls write d_offsets[0] = 0 and nothing else. */
typedef struct dskgpu_variant_params { uint32_t max_nodes, max_diff, reserved[6]; } dskgpu_variant_params;   /* 32 bytes; as dskgpu_bubble_params */
typedef struct dskgpu_variant_stats  { uint64_t n_variants, n_snps, n_multi, n_indels, n_complex, n_unitigs, stream_bytes, max_letters; } dskgpu_variant_stats; /* 64 bytes */
int dskgpu_variants(dskgpu_ctx* ctx, const dskgpu_variant_params* params, dskgpu_variant_stats* stats);
/* The kept records, on the device: d_records u32[8 * n_variants].  A null d_records: DSKGPU_E_ARG. */
int dskgpu_variants_table(dskgpu_ctx* ctx, void* d_records);
/* The kept variant stream, on the device: d_offsets u64[2 * n_variants + 1], d_bytes u8[stream_bytes].  Either may be NULL; both NULL:
 * DSKGPU_E_ARG.  capacity = the bytes d_bytes can hold; capacity < stream_bytes with a non-null d_bytes: DSKGPU_E_ARG, nothing is written. */
int dskgpu_variants_stream(dskgpu_ctx* ctx, void* d_offsets, void* d_bytes, uint64_t capacity);

/* ---- substitution errors in reads corrected against the count: the other use of a k-mer spectrum (what Bloocoo does with the output of a
 * count).  The rows of the current result are the trusted set: after dskgpu_filter_rows / _simplify / _drop_components, the rows left.
 *   STATE      Positions and validity are those of dskgpu_query_reads / dskgpu_k_enumerate.  The window ending at byte p is TRUSTED when it
 *              is valid, its canonical k-mer is a row, and that row's abundance is >= trust_min (0 and 1: any row).  state(p) = 0: no valid
 *              window ends at p; 1: valid, not trusted; 2: trusted.
 *   GAP        a maximal run [a, b] of positions of state 1, m = b - a + 1 windows.  A gap lies inside one run of bases, so the two positions
 *              beside it decide its SHAPE and its candidate byte e:
 *                interior  state(a - 1) == 2, state(b + 1) == 2 and m == k                              e = a
 *                head      state(a - 1) == 0 (or a == 0), state(b + 1) == 2 and m <= k                  e = b - k + 1
 *                tail      state(a - 1) == 2, state(b + 1) == 0 (or b is the last byte) and m <= k      e = a
 *                skipped   anything else: m > k, an interior gap shorter than k, no trusted neighbour   none
 *              In the three shaped cases the windows that contain byte e are exactly the windows of the gap.
 *   TRIAL      For each of the three bases x other than the one at e, put x at e: x WORKS when every window ending in [a, b] is then
 *              trusted.  Exactly one x works: the gap is CORRECTED, byte e becomes the letter of x in the case of the byte it replaces
 *              (letter | (old & 0x20)).  More than one: AMBIGUOUS.  None: UNFIXABLE.  Nothing is written in either case.
 * All gaps are judged against the INPUT stream and applied together.  They cannot interact: a window of one gap never contains the
 * candidate byte of another, and the states beside a gap belong to no gap.  So the result does not depend on order or scheduling, and one
 * application is final: correcting the corrected stream corrects nothing and reports the same ambiguous, unfixable and skipped gaps.
 * Limits: substitutions only, one per gap.  Indels, two errors inside one gap (closer than k: one long gap, skipped) and quality values are
 * out of scope.  One context: a rank of a group holds only the k-mers it owns, which are not the trusted set.
 * d_bytes: the stream on the device, any alignment.  params: NULL = the defaults (trust_min 0); flags and reserved must be 0.  d_out:
 * u8[nbytes] on the device, any alignment: the input with the corrected bytes replaced and every other byte copied; it may equal d_bytes
 * (in place; any other overlap is undefined) or be NULL (a dry run: statistics and states only).  d_state: u8[nbytes] or NULL: state(p) of
 * the INPUT.  stats: may be NULL.  n_valid / n_trusted: positions of state >= 1 / of state 2; n_gaps = n_interior + n_head + n_tail +
 * n_skipped; n_interior + n_head + n_tail = n_corrected + n_ambiguous + n_unfixable.
 * Like dskgpu_query_reads the call is stateless, synchronous on return, runs on the context's stream, builds the lookup index on first
 * use and encodes the stream into buffers of its own (freed before it returns: 1.375 bytes per stream byte + 25 per candidate); it touches
 * neither the reads of the context, nor the result, the stats or any graph state.  Every k in 1..128, either row order, several passes.
 * Stage times: "correct states", "correct gaps", "correct trials" (+ "query index").
 * Errors: a null ctx, a null d_bytes with nbytes > 0, non-zero flags or reserved words, a stream longer than one launch of the read frame
 * takes (as dskgpu_query_reads): DSKGPU_E_ARG; no result DSKGPU_E_STATE; a context with world_size > 1 DSKGPU_E_STATE (the text says so);
 * DSKGPU_E_NOMEM leaves everything usable.  nbytes == 0: DSKGPU_OK, all-zero stats.  A result with zero rows: every valid window is state
 * 1, nothing is corrected. */
typedef struct dskgpu_correct_params {
    uint32_t trust_min, flags; uint64_t reserved[3];
} dskgpu_correct_params;                                 /* 32 bytes; flags and reserved must be 0 */
typedef struct dskgpu_correct_stats {
    uint64_t n_valid, n_trusted, n_gaps, n_interior, n_head, n_tail, n_skipped, n_corrected, n_ambiguous, n_unfixable, reserved[6];
} dskgpu_correct_stats;                                  /* 128 bytes */
int dskgpu_correct_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const dskgpu_correct_params* params, void* d_out, void* d_state,
                         dskgpu_correct_stats* stats);

/* ---- per-read abundance summaries and read selection: a count is also a spectrum that says something about each READ.  The calls above
 * answer per position (dskgpu_query_reads, dskgpu_correct_reads, dskgpu_thread_place); these answer per read and take reads out of a
 * stream: "keep the reads whose median k-mer abundance is between 5 and 80", "drop the reads with fewer than 90 % solid k-mers", "drop the
 * reads that hit this contaminant set at all" -- khmer's filter-abund and slice-reads-by-coverage, the static half of digital
 * normalisation, BBDuk-style screening -- without copying 4 bytes per base to the host.
 *   RECORD     The stream is cut at the bytes 0x0A.  Record i is the bytes between the (i-1)-th and the i-th '\n', with neither included.
 *              start_i is its first byte and len_i its length.  A record may be empty (two '\n' in a row, or a '\n' at byte 0).
 *              n_records = the number of '\n', plus 1 when nbytes > 0 and the last byte is not '\n'.  Any other non-ACGT byte (N, '\r',
 *              IUPAC) lies inside a record and only ends windows, as the input convention says.  A '\n' ends every window, so no window
 *              spans two records.
 *   VALUE      of a position p in a record.  valid(p) is exactly dskgpu_k_enumerate's validity.  For a valid p, a(p) is what
 *              dskgpu_query_reads answers: the row's abundance, or 0 when the k-mer is no row.  p is SOLID when it is valid and
 *              a(p) >= max(trust_min, 1).
 *   SUMMARY    of record i, 32 bytes, in this order:
 *                start    u64  start_i
 *                sum      u64  sum of a(p) over the valid positions of the record
 *                len      u32  len_i
 *                n_valid  u32  valid positions
 *                n_solid  u32  SOLID positions
 *                median   u32  the values a(p) of the valid positions, sorted ascending: the element of index n_valid / 2 (integer
 *                              division, khmer's convention).  0 when n_valid == 0.
 *              A record longer than 2^32 - 1 bytes gives DSKGPU_E_ARG, and the error text says so.  The stream's length limit is that of
 *              dskgpu_query_reads.
 *   RULE       Record i is KEPT when all of the following hold: n_valid >= min_valid; median >= median_min; median_max == 0 or
 *              median <= median_max; solid_den == 0 or (u64)n_solid * solid_den >= (u64)solid_num * n_valid.  With flag bit 0
 *              (DSKGPU_READS_INVERT) the answer is flipped.  A null rule keeps everything.  Other flag bits or non-zero reserved words
 *              give DSKGPU_E_ARG.
 *   SELECTION  The kept records, in stream order, each followed by one '\n'.  out_bytes = sum over kept records of len + 1.
 *              out_records = the number of kept records.  A last record without a '\n' gets one.  Selecting with every flag set from a
 *              stream that ends in '\n' reproduces the stream.
 * dskgpu_read_summaries builds the table of the stream's summaries and keeps it in the context, the way a threading is kept.  It runs on the
 * context's stream, is synchronous on return, builds the lookup index on first use and encodes the stream into scratch of its own, freed
 * before it returns; it leaves the reads (a kept encoding included), the result, the stats, the sender state and every graph table alone.
 * Every k in 1..128, either row order, several passes.  One context: a rank of a group holds only the k-mers it owns, so world_size > 1
 * gives DSKGPU_E_STATE, as for the correction.  d_bytes: the stream on the device, any alignment.  params: NULL = the defaults (trust_min 0);
 * flags and reserved must be 0.  stats (may be NULL): n_records; n_empty = the records with n_valid == 0; n_valid and n_solid = the sums over
 * the records; max_len = the longest record.
 * Lifetime of the kept table: dropped by the next count, by dskgpu_filter_rows and everything built on it (dskgpu_clip_tips / _pop_bubbles /
 * _remove_connections / _simplify / _simplify_all / _drop_components), by the next dskgpu_read_summaries and by dskgpu_destroy.
 * Memory: while it runs, the 2-bit form of the stream (0.375 bytes per stream byte) + 4.125 bytes per stream byte for the values and the
 * valid bits + 8 bytes per record for the record ends and 8 per record longer than the wave path takes (+ 16 bytes per 4096 stream bytes of
 * block sums); what it keeps is 32 bytes per record.  dskgpu_select_reads takes, and frees before it returns, 24 bytes per record (+ the
 * block sums).  A stream too big for the free HBM can be summarised and selected in pieces cut behind any '\n'.
 * Stage times: "read values", "read records", "read summaries" (dskgpu_read_summaries), "read records", "read select"
 * (dskgpu_select_reads), plus "query index" when the call builds the index.
 * Errors: a null ctx, a null d_bytes with nbytes > 0, non-zero flags or reserved words, a stream longer than one launch of the read frame
 * takes (as dskgpu_query_reads), a record longer than 2^32 - 1 bytes: DSKGPU_E_ARG; no result DSKGPU_E_STATE; a context with world_size > 1
 * DSKGPU_E_STATE (the text says so); a table or marks call when no table is kept DSKGPU_E_STATE; DSKGPU_E_NOMEM leaves the context, its
 * result and what was built before usable.  After a failed dskgpu_read_summaries no table is kept.  nbytes == 0: DSKGPU_OK, all-zero stats,
 * a table of zero records is kept: the table call writes nothing, the marks call gives all-zero stats.  A result with zero rows: every value
 * is 0, so every sum, n_solid and median is 0; n_valid is still counted. */
#define DSKGPU_READS_INVERT 1u                           /* dskgpu_read_rule.flags bit 0: keep what the rule would drop */
typedef struct dskgpu_read_summary_params { uint32_t trust_min, flags; uint64_t reserved[3]; } dskgpu_read_summary_params;     /* 32 bytes; flags and reserved must be 0 */
typedef struct dskgpu_read_summary_stats  { uint64_t n_records, n_empty, n_valid, n_solid, max_len, reserved[3]; } dskgpu_read_summary_stats;  /* 64 bytes */
typedef struct dskgpu_read_rule           { uint32_t min_valid, median_min, median_max, solid_num, solid_den, flags; uint64_t reserved; } dskgpu_read_rule; /* 32 bytes */
typedef struct dskgpu_read_mark_stats     { uint64_t n_records, n_kept, kept_bytes, kept_valid, reserved[4]; } dskgpu_read_mark_stats;      /* 64 bytes; kept_bytes = sum of len + 1 */
int dskgpu_read_summaries(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const dskgpu_read_summary_params* params, dskgpu_read_summary_stats* stats);
/* The kept table, on the device: d_records = n_records summaries of 32 bytes, 8-byte aligned.  A null d_records: DSKGPU_E_ARG. */
int dskgpu_read_summaries_table(dskgpu_ctx* ctx, void* d_records);
/* The RULE applied to the kept table, which stays as it is.  d_keep: u8[n_records] on the device <- 1 (kept) or 0; may be NULL, for the stats
 * only.  stats may be NULL, but not both: DSKGPU_E_ARG.  rule: NULL keeps everything.  stats: n_records, n_kept, kept_bytes = out_bytes of
 * the selection by these marks, kept_valid = the sum of n_valid over the kept records. */
int dskgpu_read_marks(dskgpu_ctx* ctx, const dskgpu_read_rule* rule, void* d_keep, dskgpu_read_mark_stats* stats);
/* The SELECTION.  Stateless: it needs no result and no kept table, finds the records of the stream itself, works on a context that has never
 * counted and leaves everything in the context alone.  d_keep: u8[n_records] on the device, non-zero = keep; from dskgpu_read_marks or the
 * caller's own -- a caller with paired files ANDs the two files' flags and selects both streams, and the pairs stay in step.  n_records must
 * be the stream's own count: anything else is DSKGPU_E_ARG (nbytes == 0: n_records 0, nothing is written, *out_bytes = *out_records = 0).
 * d_out == NULL is a sizing run: only *out_bytes / *out_records are written (either may be NULL).  capacity < out_bytes with a non-null
 * d_out: DSKGPU_E_ARG, nothing is written to d_out and *out_bytes is set to the need.  d_out must not overlap d_bytes.  Any alignment of
 * either pointer.  A null ctx, a null d_bytes with nbytes > 0, a null d_keep with n_records > 0, a stream longer than dskgpu_query_reads
 * takes: DSKGPU_E_ARG. */
int dskgpu_select_reads(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const void* d_keep, uint64_t n_records, void* d_out, uint64_t capacity,
                        uint64_t* out_bytes, uint64_t* out_records);

/* ---- sample colours for rows, unitigs and variants: everything above answers questions about ONE pooled set of reads.  The consumers
 * these calls were modelled on are mostly multi-sample tools: DiscoSnp genotypes every bubble per sample, Cortex, Bifrost and kmtricks keep
 * a colour per k-mer, a GFA viewer draws per-sample coverage on the unitigs, a differential analysis asks which unitigs are private to one
 * sample.  These calls turn a read stream with bank boundaries into a row x colour count matrix and reduce it onto the unitigs.  Alphabet,
 * window validity and positions are exactly those of dskgpu_k_enumerate / dskgpu_query_reads; "row" is as dskgpu_query_kmers means it.
 *   COLOURS         A context holds at most one colour matrix.  It has n_colors columns, 1..64.  The matrix is u32 C[n_rows][n_colors],
 *                   row-major, in result order, zeroed by dskgpu_colors_begin.
 *   BANK            of a position.  In one dskgpu_colors_add call with end_offsets[0..n_banks), position p lies in bank b when b is the
 *                   least index with p < end_offsets[b].  end_offsets is a host array, non-decreasing, with
 *                   end_offsets[n_banks-1] <= nbytes.  Positions at or beyond the last end have no bank and are not counted.  The colour
 *                   of p is first_color + b.  An empty bank (two equal ends) is legal.  The bank belongs to the byte the window ENDS at:
 *                   in a stream whose banks each end with '\n', no window crosses a boundary.
 *   CELL            C[r][c] is the number of positions p -- of any dskgpu_colors_add call since dskgpu_colors_begin -- that have colour
 *                   c, whose window (the one ending at p) is valid and whose canonical k-mer is row r.  A window over a palindromic row
 *                   (even k) counts once.  Arithmetic is modulo 2^32: fewer than 2^32 bytes per colour cannot wrap.  Integer adds
 *                   commute, so the matrix does not depend on scheduling.
 *   MASK            mask(min_count)[r] is a u64 whose bit c is set iff C[r][c] >= min_count.  min_count >= 1; 0 is DSKGPU_E_ARG.
 *   UNITIG COLOURS  sum[u][c] is the sum of C[r][c] over the rows with unitig[r] == u (u64, exact); all[u] is the AND of those rows' masks,
 *                   any[u] the OR.  sum[u][c] / L[u] is the sample's mean coverage of the unitig; `all` marks the unitigs that a sample
 *                   covers end to end.
 *   VARIANT COLOURS For variant v with alleles A, B (oriented unitigs of dskgpu_variants_table): vsum[v][0][c] = sum[A >> 1][c] and
 *                   vsum[v][1][c] = sum[B >> 1][c] -- DiscoSnp's per-sample allele coverage.  A gather from the unitig table: no call of
 *                   its own (KmerCounter.variants_colors_tensor does it).
 * The calls run on the context's stream and are synchronous on return.  They change nothing else in the context: the reads, a kept
 * encoding, the result, the stats, the sender state and a kept threading stay as they are.  dskgpu_colors_add builds the lookup index on
 * first use and encodes the stream into scratch of its own (0.375 bytes per stream byte), freed before it returns; the matrix takes
 * 4 * n_rows * n_colors bytes.  d_bytes: the stream on the device, any alignment, any length (a long stream takes several launches).
 * Lifetime: the matrix lives in the context next to the read summaries.  It is dropped, and its memory freed, by the next count, by
 * dskgpu_filter_rows and everything built on it (dskgpu_clip_tips / _pop_bubbles / _remove_connections / _simplify / _simplify_all /
 * _drop_components) and by dskgpu_destroy; a second dskgpu_colors_begin replaces it.  The intended order is count, clean the graph, then
 * colour.  After the rows change, add / rows / unitigs without a new begin are DSKGPU_E_STATE.
 * Which results are served: every k (1..128), either row order, DSKGPU_F_NO_SORT, several passes, the per-bank modes and a rank's rows
 * (world_size > 1) for begin / add / rows, which only need the lookup index.  dskgpu_colors_unitigs needs the compaction: it builds it on
 * first use as the other graph calls do, and is DSKGPU_E_STATE on a rank of a group.
 * Stage times: "colors" (dskgpu_colors_add), "color unitigs" (dskgpu_colors_unitigs), plus "query index" / "unitigs" when the call builds them.
 * Errors: DSKGPU_E_ARG: a null ctx; n_colors 0 or > 64; first_color + n_banks > n_colors; n_banks == 0 with nbytes > 0; decreasing ends, or
 * an end above nbytes; a null d_bytes or end_offsets with nbytes > 0; d_counts and d_mask both null, or all three outputs of _unitigs null;
 * min_count == 0.  DSKGPU_E_STATE: no result, or no begin (a call out of order is reported before first_color + n_banks is compared with
 * n_colors).  nbytes == 0: DSKGPU_OK, nothing is done, all-zero stats.  DSKGPU_E_NOMEM leaves the context and everything built
 * usable; after a failed dskgpu_colors_begin no matrix is kept.  A result with zero rows: begin and add succeed, n_placed is 0, and nothing
 * is written by the copy calls. */
typedef struct dskgpu_color_stats { uint64_t n_valid, n_placed, n_rows, n_colors, reserved[4]; } dskgpu_color_stats;   /* 64 bytes */
int dskgpu_colors_begin(dskgpu_ctx* ctx, uint32_t n_colors);
/* stats (may be NULL): the counts of this one call.  n_valid = the valid windows that have a bank; n_placed = those of them that are rows,
 * which is the amount this call added to the matrix; n_rows, n_colors = the shape of the matrix. */
int dskgpu_colors_add(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, const uint64_t* end_offsets, uint32_t n_banks, uint32_t first_color,
                      dskgpu_color_stats* stats);
/* d_counts: u32[n_rows * n_colors] on the device <- the matrix; d_mask: u64[n_rows] <- mask(min_count); either may be NULL, not both.
 * d_counts 4-byte aligned (16-byte aligned with n_colors a multiple of 4: copied with 16-byte accesses), d_mask 8-byte aligned. */
int dskgpu_colors_rows(dskgpu_ctx* ctx, uint32_t min_count, void* d_counts, void* d_mask);
/* d_sum: u64[n_unitigs * n_colors], d_all / d_any: u64[n_unitigs], on the device, 8-byte aligned; any may be NULL, not all three. */
int dskgpu_colors_unitigs(dskgpu_ctx* ctx, uint32_t min_count, void* d_sum, void* d_all, void* d_any);

/* ---- comparing the samples, choosing rows by colour, keeping colours across a row change: the calls above look at one row or one unitig of
 * the colour matrix at a time.  These look at the matrix as a whole.  dskgpu_colors_pairs reduces it to three n_colors x n_colors matrices,
 * from which Jaccard, Sorensen, Ochiai, Kulczynski, Bray-Curtis and the abundance-weighted distances between samples follow (what Simka
 * computes; what kmtricks and Mash-style workflows derive from a k-mer matrix; KmerCounter's sample_distances does the arithmetic) -- one pass
 * over a matrix that already lies in device memory instead of a copy of 4 * n_rows * n_colors bytes.  dskgpu_colors_marks turns a rule on a
 * row's colours into the byte per row that dskgpu_filter_rows takes (the k-mers private to some samples, present in at least m, the core, the
 * accessory part), as dskgpu_read_marks does for reads.  dskgpu_colors_load makes a matrix of the caller's the kept one: a caller that saved
 * the matrix with dskgpu_colors_rows before a row change puts it back, gathered to the kept rows, instead of streaming every read again.
 *   THRESHOLDED CELL  C'[r][c] = C[r][c] if C[r][c] >= min_count, else 0.  min_count >= 1; 0 is DSKGPU_E_ARG.  mask(min_count)[r] has bit c
 *                     set iff C'[r][c] > 0.
 *   SELECTED          Row r is selected when d_select is NULL or d_select[r] != 0.  d_select: u8[n_rows] on the device, any alignment (the
 *                     form of dskgpu_colors_marks' and dskgpu_filter_rows' bytes).
 *   PAIR MATRICES     u64[n_colors][n_colors] each, row-major, on the device, 8-byte aligned; the sums run over the selected rows.
 *                       shared[i][j]  = the number of rows with C'[r][i] > 0 and C'[r][j] > 0.  Symmetric; shared[i][i] is sample i's
 *                                       distinct k-mers.
 *                       cross[i][j]   = the sum of C'[r][i] over the rows with C'[r][j] > 0.  Not symmetric; cross[i][i] is sample i's
 *                                       total, and cross[i][j] / cross[i][i] is Simka's U.
 *                       min_sum[i][j] = the sum of min(C'[r][i], C'[r][j]).  Symmetric; min_sum[i][i] == cross[i][i].
 *                     Any of the three may be NULL, but not all three.  Every entry is exact in 64 bits and does not depend on scheduling:
 *                     a cell may be 2^32 - 1, and no partial sum is held in anything that can wrap (integer adds only).
 *   RULE              With m = mask(rule.min_count)[r], keep0 is true exactly when (m & need_all) == need_all, (m & need_none) == 0,
 *                     popcount(m) >= min_present, and max_present == 0 or popcount(m) <= max_present.  d_keep[r] (u8) = keep0 XOR flag
 *                     bit 0 (DSKGPU_COLORS_INVERT): 1 or 0, the form dskgpu_filter_rows takes.
 * State: the three calls need only the kept matrix, keep nothing in the context and change nothing in it (dskgpu_colors_load changes the
 * matrix itself).  So they serve every k, either row order, DSKGPU_F_NO_SORT, several passes and a rank's rows (world_size > 1).  The ranks
 * of a group partition the k-mers, so the job-wide pair matrices are the element-wise sums of the ranks' matrices.  The calls run on the
 * context's stream and are synchronous on return.  dskgpu_colors_load does what dskgpu_colors_begin does -- same lifetime, same errors, it
 * replaces a kept matrix -- but the new matrix is a copy of d_counts: u32[n_rows][n_colors] of the current result, row-major, on the device,
 * 4-byte aligned.
 * Stage times: "color pairs", "color marks", "color load".
 * Errors: DSKGPU_E_ARG: a null ctx; min_count == 0; all three outputs null; n_colors 0 or > 64; a null d_counts while there are rows; a null
 * rule; unknown flag bits; bits of need_all or need_none at or above n_colors; a null d_keep while there are rows.  DSKGPU_E_STATE: no kept
 * matrix (pairs, marks); no result (load).  A result with zero rows: DSKGPU_OK; the pair matrices are zeroed, the stats are all zero, nothing
 * is written to d_keep, and dskgpu_colors_load takes a null d_counts. */
typedef struct dskgpu_color_pair_stats { uint64_t n_rows, n_selected, n_present, n_colors, reserved[4]; } dskgpu_color_pair_stats;   /* 64 bytes */
/* stats (may be NULL): n_rows, n_colors = the shape of the matrix; n_selected = the selected rows; n_present = the selected rows with some
 * C'[r][c] > 0. */
int dskgpu_colors_pairs(dskgpu_ctx* ctx, uint32_t min_count, const void* d_select, void* d_shared, void* d_cross, void* d_min_sum,
                        dskgpu_color_pair_stats* stats);
int dskgpu_colors_load(dskgpu_ctx* ctx, const void* d_counts, uint32_t n_colors);
#define DSKGPU_COLORS_INVERT 1u                          /* dskgpu_color_rule.flags bit 0: keep what the rule would drop */
typedef struct dskgpu_color_rule { uint64_t need_all, need_none; uint32_t min_count, min_present, max_present, flags; } dskgpu_color_rule;   /* 32 bytes */
typedef struct dskgpu_color_mark_stats { uint64_t n_rows, n_kept, reserved[6]; } dskgpu_color_mark_stats;                                    /* 64 bytes */
/* stats (may be NULL): n_rows; n_kept = the rows whose byte is 1. */
int dskgpu_colors_marks(dskgpu_ctx* ctx, const dskgpu_color_rule* rule, void* d_keep, dskgpu_color_mark_stats* stats);

/* ---- saved rows loaded into a context, counts merged: everything above starts from a count of reads made by this context.  The reference's
 * whole point is to leave a reusable k-mer table, and its users add the abundances of equal k-mers of two tables (Jellyfish `merge`, KMC
 * `kmc_tools simple union`, banks counted on different days).  A LOAD IS A COUNT WHOSE INPUT IS (k-mer, abundance) PAIRS INSTEAD OF READS:
 * equal k-mers are combined, the context's abundance_min / abundance_max filter the combined value, the histogram is taken over all distinct
 * k-mers, the kept rows become the result in the global order, and every later call (lookups, graph, filter, colours) works as after a count.
 *   input      d_kmers: n values of words = ceil(k / 32) u64 each, row-major, least-significant word first (the layout of
 *              dskgpu_partition_copy, dskgpu_query_kmers and dskgpu_k_enumerate), 8-byte aligned; d_abundance: n u32, 4-byte aligned.  Both on
 *              the device, in any order, with any number of repeats; both are left as they were.  They must NOT be memory the context owns
 *              (dskgpu_result_device's arrays among it): that is the caller's duty.  n <= 2^32 - 2, the limit of the lookup index and of this
 *              call: more is DSKGPU_E_ARG.  For k > 64 the limit is n < 2^32 - 65536, that of the row order of four-word rows.
 *   validity   every value < 4^k and canonical -- value <= revcomp(value) in the order A=0 C=1 T=2 G=3; the palindromes of an even k are
 *              valid -- and every abundance >= 1; with DSKGPU_LOAD_UNIQUE no value may repeat.  A violation is DSKGPU_E_ARG, and the error
 *              text names the LOWEST offending input index and what is wrong with it.  A repeat under DSKGPU_LOAD_UNIQUE is looked for once
 *              every row is valid by itself; the offending index is then the lowest i whose value also stands at some j < i, and the text
 *              gives the value.  Validation reads only the input: on this error the previous result and everything built on it are untouched.
 *   combine    DSKGPU_LOAD_SUM: the abundances of equal values added in 64 bits and stored saturated at 2^32 - 1; _MAX, _MIN: the largest /
 *              smallest; _UNIQUE: equal values are an error.
 *   result     the distinct values with abundance_min <= combined <= abundance_max, ascending by value over all rows, struct-of-arrays in
 *              buffers of the context, exactly as a global-order count leaves them.  A load ignores DSKGPU_F_PARTITION_ORDER and
 *              DSKGPU_F_NO_SORT: the loaded result is always in the global order, its partitions are the n_rows * p / P ranges with
 *              P = nb_partitions or 4.  A later dskgpu_count follows the flags again.
 *   record     the load REPLACES the count's record: dskgpu_histogram = hist[min(combined, histo_max)] over all distinct values;
 *              dskgpu_get_stats: n_bytes 0, n_kmers = the exact 64-bit sum of the INPUT abundances (not of the saturated ones), n_distinct =
 *              the distinct values, n_solid = the rows kept, n_partitions as above, sort_fallback as the row order reports it, every other
 *              field 0; the 2-D histogram is forgotten.
 *   stats      (may be NULL) n_in = n; n_distinct, n_rows, n_kmers as in the record; n_below / n_above: the distinct values filtered out on
 *              either side; n_saturated: the distinct values whose SUM exceeded 2^32 - 1; sorted_input: 1 when the input was already strictly
 *              ascending (the order step is then skipped).
 * State: where a count would drop the old result it goes here too, with the index, compaction, threading, variants, summaries, colours and
 * filtered rows.  The context's reads, a kept encoding and the sender state are untouched: load, then dskgpu_count, gives what the count
 * alone gives.  n == 0: DSKGPU_OK, a result with zero rows and an all-zero histogram; null arrays are allowed then.  The call runs on the
 * context's stream and is synchronous on return.  Stage times: "load check", "load order", "load combine".
 * Errors: DSKGPU_E_ARG: a null ctx; a null array while n > 0; a misaligned array; combine > 3; n above the limit; an invalid row.
 * DSKGPU_E_STATE: a context of a group (world_size > 1): a rank owns a slice of the k-mer space and a load knows nothing of it.
 * DSKGPU_E_NOMEM / DSKGPU_E_DEVICE: as after a failed count, there is no result. */
#define DSKGPU_LOAD_SUM    0u   /* equal k-mers: abundances added in 64 bits, stored saturated at 2^32 - 1 */
#define DSKGPU_LOAD_MAX    1u
#define DSKGPU_LOAD_MIN    2u
#define DSKGPU_LOAD_UNIQUE 3u   /* equal k-mers are an error (DSKGPU_E_ARG) */
typedef struct dskgpu_load_stats {
    uint64_t n_in, n_distinct, n_rows, n_below, n_above, n_kmers, n_saturated, sorted_input;
} dskgpu_load_stats;            /* 64 bytes */
int dskgpu_load_rows(dskgpu_ctx* ctx, const void* d_kmers, const void* d_abundance, uint64_t n, uint32_t combine, dskgpu_load_stats* stats);

/* ---- the same call on N GPUs of one node, inside ONE process (what `dsk -nb-gpus N` runs): the reference's
 * single `execute()` (src/DSK.cpp:55-60) still leaves ONE storage with a flat list of solid partitions
 * (utils/dsk2ascii.cpp:61,77).  A group owns one ctx per rank (world_size = n_ranks, rank r on devices[r], its own
 * stream and host thread).  Feed every rank its share of the reads through dskgpu_group_ctx(g, r) with the input
 * calls above (any split of whole records is valid: counting is a group-by on the canonical k-mer), then
 * dskgpu_group_count runs mg_scatter -> exchange -> mg_count on all ranks at once.  The exchange is an
 * all-to-all-v of super-k-mer records: grouped ncclSend / ncclRecv over RCCL (one communicator per rank from
 * ncclCommInitAll; librccl is loaded on first use) when every rank has its own device, device-to-device copies
 * when ranks share a device (RCCL refuses duplicate devices: the multi-rank tests on a 1-GPU box).
 * DSKGPU_GROUP_TRANSPORT=rccl|copy (environment, read at create) overrides the choice.  n_ranks: power of two <= 64.
 * cfg->device / world_size / rank are ignored (set per rank).  Results: per rank through dskgpu_group_ctx, or merged:
 * the histogram is the element-wise sum; global partition P = p * n_ranks + r is local partition p of rank r. */
typedef struct dskgpu_group dskgpu_group;
int  dskgpu_group_create(const dskgpu_config* cfg, const int32_t* devices, uint32_t n_ranks, dskgpu_group** out);
void dskgpu_group_destroy(dskgpu_group* g);
const char* dskgpu_group_last_error(const dskgpu_group* g);   /* g may be NULL: create-time error */
uint32_t dskgpu_group_size(const dskgpu_group* g);
dskgpu_ctx* dskgpu_group_ctx(dskgpu_group* g, uint32_t rank);
const char* dskgpu_group_transport(const dskgpu_group* g);     /* "rccl" or "copy" */
int dskgpu_group_count(dskgpu_group* g);
uint64_t dskgpu_group_exchanged_words(const dskgpu_group* g);  /* 8-byte words that changed rank in the last count */
/* steps of the last count that ran in slices -- exchange overlapped with the sender and the receiver's level 1 (dskgpu_mg_slices_*;
 * DSKGPU_GROUP_SLICES = slices per step, default 4, < 2 = every step in one piece); 0 when the input took the one-piece path */
uint32_t dskgpu_group_sliced_steps(const dskgpu_group* g);
int dskgpu_group_histogram(const dskgpu_group* g, uint64_t* out, uint32_t nbins);
/* Per-bank modes (solidity_kind != sum, DSKGPU_F_HISTO2D; banks = dskgpu_next_bank on EVERY rank's context at the same
 * points of the stream): dskgpu_group_count counts the banks one by one with one repartition table, every rank applies the
 * solidity kind to the k-mers it owns; the 2-D histogram is the element-wise sum (README.md:98-102). */
int dskgpu_group_histogram2d(const dskgpu_group* g, uint64_t* out, uint32_t nrows);
int dskgpu_group_get_stats(const dskgpu_group* g, dskgpu_stats* out);   /* sums over the ranks */
uint32_t dskgpu_group_num_partitions(const dskgpu_group* g);
uint64_t dskgpu_group_partition_size(const dskgpu_group* g, uint32_t P);
int dskgpu_group_partition_copy(const dskgpu_group* g, uint32_t P, uint64_t* kmers, uint32_t* abundance);

/* ---- kernel-level entry points used by the parity tests (device pointers) */
/* ASCII -> 2-bit packed words + invalid mask: (nbytes + 31) / 32 words are written to each of d_packed (u64) and d_invalid (u32),
 * and nothing behind them.  Word w holds bytes 32 w .. 32 w + 31; byte 32 w + j is "base j" of the word.
 *   d_packed[w]   the code of base j in bits 63 - 2 j .. 62 - 2 j (base 0 in the two highest bits): A = 0, C = 1, T = 2, G = 3,
 *                 either case
 *   d_invalid[w]  bit 31 - j set iff byte 32 w + j is none of the eight letters ACGTacgt -- every other value of the 256, the
 *                 control characters and the values from 0x80 on included -- or lies at or beyond nbytes: the pad of the last
 *                 word reads as invalid
 * The two code bits under an invalid position are unspecified: read d_packed under the mask of the valid positions only.
 * d_bytes needs no alignment (a 16-byte aligned stream takes wider loads; the result is the same). */
int dskgpu_k_encode(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_packed, void* d_invalid);
/* Canonical k-mer (words = ceil(k/32) u64, LSW first) + validity byte for the window ending at every byte. */
int dskgpu_k_enumerate(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_kmers, void* d_valid);
/* Minimizer (u32) of the window ending at every byte (0 when invalid). */
int dskgpu_k_minimizers(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes, void* d_minim, void* d_valid);

#ifdef __cplusplus
}
#endif
#endif
