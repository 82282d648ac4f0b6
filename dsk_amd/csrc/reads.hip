// reads.hip -- the read stream a context owns (dskgpu_ctx::reads, engine.h: ReadStream): bytes pushed from the host through two pinned
// staging buffers (dskgpu_push_reads), file text parsed on the device (dskgpu_push_raw, rawparse.h), the stream's buffer and length
// (dskgpu_reserve_reads, _stream_bytes, _rewind_reads) and the read set of the caller's that takes its place (dskgpu_set_reads_device).
// What a count reads is ctx->d_reads / n_bytes, set here whenever the stream changes: the count path never looks at who owns the bytes.
#include <system_error>
#include <thread>

#include "engine.h"
#include "rawparse.h"

#define PIN_CHUNK ((size_t)32 << 20)
static_assert(PIN_CHUNK == ((size_t)32 << 20), "launch_raw_chunk's capacity check is written for 32 MB pieces");
static_assert(((size_t)32 << 20) / RP_BLOCK <= (size_t)RP_NT * RP_SCAN_PER, "k_rp_scan walks the block summaries of one staging piece (PIN_CHUNK) with RP_SCAN_PER per thread");
template <int FMT>
static void launch_raw_chunk(dskgpu_ctx* ctx, u32 n, uint8_t* out) {
    ReadStream& r = ctx->reads;
    const u32 nb = (n + RP_BLOCK - 1) / RP_BLOCK;
    const unsigned char* in = r.raw_in.as<unsigned char>();
    RawState* st = r.raw_state.as<RawState>();
    hipLaunchKernelGGL((k_rp_count<FMT>), dim3(nb), dim3(RP_NT), 0, ctx->stream, in, n, r.raw_blk.as<RpBlock>());
    hipLaunchKernelGGL((k_rp_scan<FMT>), dim3(1), dim3(RP_NT), 0, ctx->stream, in, n, nb, r.raw_blk.as<RpBlock>(), st,
                       r.raw_boff.as<unsigned long long>(), r.raw_bstate.as<u32>(), out);
    hipLaunchKernelGGL((k_rp_write<FMT>), dim3(nb), dim3(RP_NT), 0, ctx->stream, in, n, r.raw_boff.as<unsigned long long>(),
                       r.raw_bstate.as<u32>(), st, out);
}
// The raw pushes' result: the stream's length comes back from the device (the one synchronisation of a raw ingest), the terminator is set.
int raw_finish(dskgpu_ctx* ctx, u64* lines) {
    ReadStream& r = ctx->reads;
    if (!r.raw_pending) return DSKGPU_OK;
    RawState s;
    CK(hipMemcpyAsync(&s, r.raw_state.p, sizeof(RawState), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    r.raw_pending = false;
    uint8_t* dst = r.own.as<uint8_t>();
    if (!rp_file_ok(s)) s.bad = 1;      // (the last file, now that it is complete: its quality lines must add up to its sequence lines)
    if (s.bad) {             // the text is not what the device parser handles: the raw pushes are dropped, the stream is what it was before them
        r.len = r.raw_base;
        ctx->d_reads = dst; ctx->n_bytes = r.len;
        return fail(ctx, DSKGPU_E_FORMAT, "dskgpu_push_raw: the text is not 4-line FASTQ / FASTA as declared (the raw pushes were dropped: parse on the host and push the reads)");
    }
    if (s.out_len + 1 > r.own.cap) return fail(ctx, DSKGPU_E_STATE, "dskgpu_push_raw: stream longer than its bound");
    CK(hipMemsetAsync(dst + s.out_len, '\n', 1, ctx->stream));
    r.len = s.out_len + 1;
    if (lines) *lines = s.recs;
    ctx->d_reads = dst; ctx->n_bytes = r.len; ctx->enc_keep = false; ctx->reads_changed();
    return DSKGPU_OK;
}
// pageable -> pinned: one thread copies ~10 GB/s on the host this was measured on, the link takes 55: big pieces are copied by up to eight (a memory-mapped file's pages are also faulted in by the copy)
static void stage_copy(void* dst, const void* src, size_t n) {
    const unsigned T = n >= ((size_t)16 << 20) ? 8u : n >= ((size_t)8 << 20) ? 4u : n >= ((size_t)2 << 20) ? 2u : 1u;
    if (T == 1) { std::memcpy(dst, src, n); return; }
    const size_t per = (((n + T - 1) / T) + 4095) & ~(size_t)4095;          // T * per >= n
    auto part = [=](unsigned t) { const size_t a = (size_t)t * per; if (a < n) std::memcpy((char*)dst + a, (const char*)src + a, std::min(per, n - a)); };
    std::thread th[7];
    unsigned started = 1;
    try { for (; started < T; ++started) th[started - 1] = std::thread(part, started); }
    catch (const std::system_error&) {}                      // (no more threads to be had: the parts that got none are copied here)
    part(0);
    for (unsigned t = started; t < T; ++t) part(t);
    for (unsigned t = 1; t < started; ++t) th[t - 1].join();
}
static int ensure_pinned(dskgpu_ctx* ctx) {      // the two pinned staging buffers of the pushes (also set up by dskgpu_reserve_reads: off the first push's path)
    ReadStream& r = ctx->reads;
    if (r.pin[0] && r.pin[1]) return DSKGPU_OK;
    for (int i = 0; i < 2; ++i) {
        if (!r.pin[i]) CK(hipHostMalloc(&r.pin[i], PIN_CHUNK, hipHostMallocDefault));
        if (!r.pin_ev[i]) CK(hipEventCreateWithFlags(&r.pin_ev[i], hipEventDisableTiming));
    }
    return DSKGPU_OK;
}
// The next piece, of at most PIN_CHUNK, of the `left` pageable bytes at src -> one of the two pinned staging buffers -> dst in HBM; -> *len: the piece's length.  The CPU
// copy of one piece overlaps the DMA of the previous one (a direct pageable hipMemcpy reached 4.5 GB/s); what the caller enqueues next runs behind this piece's DMA.
static int stage_piece(dskgpu_ctx* ctx, const char* src, u64 left, uint8_t* dst, size_t* len) {
    ReadStream& r = ctx->reads;
    { const int e = ensure_pinned(ctx); if (e) return e; }
    const int slot = r.pin_next;       // (alternates ACROSS calls too: the copy of this call's first piece overlaps the DMA of the last call's last one)
    *len = (size_t)std::min<u64>(PIN_CHUNK, left);
    if (r.pin_used[slot]) CK(hipEventSynchronize(r.pin_ev[slot]));
    stage_copy(r.pin[slot], src, *len);
    CK(hipMemcpyAsync(dst, r.pin[slot], *len, hipMemcpyHostToDevice, ctx->stream));
    CK(hipEventRecord(r.pin_ev[slot], ctx->stream));
    r.pin_used[slot] = true; r.pin_next ^= 1;
    return DSKGPU_OK;
}
// The stream buffer must hold `need` bytes; its first `keep` bytes are kept.  roomy (the pushes): a buffer that grows becomes at least
// twice as large and never less than 256 MB; else (a reservation) exactly `need`.
static int stream_hold(dskgpu_ctx* ctx, u64 need, u64 keep, bool roomy) {
    DevBuf& own = ctx->reads.own;
    if (need <= own.cap) return DSKGPU_OK;
    DevBuf nb;
    CK(nb.ensure(roomy ? std::max<u64>(need, std::max<u64>(own.cap * 2, (u64)256 << 20)) : need));
    if (keep) CK(hipMemcpyAsync(nb.p, own.p, keep, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    own.release();
    own = nb;
    return DSKGPU_OK;
}

extern "C" {
int dskgpu_push_reads(dskgpu_ctx* ctx, const char* bytes, uint64_t nbytes) {
    if (!ctx || (!bytes && nbytes)) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    ReadStream& r = ctx->reads;
    if (r.raw_pending) { const int e = raw_finish(ctx, nullptr); if (e) return e; }
    { const int e = stream_hold(ctx, r.len + nbytes + 1, r.len, true); if (e) return e; }
    uint8_t* dst = r.own.as<uint8_t>();
    size_t len = 0;
    for (u64 off = 0; off < nbytes; off += len) { const int e = stage_piece(ctx, bytes + off, nbytes - off, dst + r.len + off, &len); if (e) return e; }
    CK(hipMemsetAsync(dst + r.len + nbytes, '\n', 1, ctx->stream));
    // (no synchronisation here: the caller's bytes were copied to the pinned staging buffers above, and everything that reads the
    //  device copy -- the count, a later growth of the buffer -- is ordered behind the DMA on the context's stream.  A bank that
    //  hands over a few MB per call keeps the link busy this way instead of paying a round trip per call.)
    r.len += nbytes + 1;
    ctx->d_reads = dst; ctx->n_bytes = r.len; ctx->enc_keep = false; ctx->reads_changed();
    return DSKGPU_OK;
}

int dskgpu_raw_finish(dskgpu_ctx* ctx, uint64_t* stream_bytes, uint64_t* records) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    u64 ln = 0;
    const int rc = raw_finish(ctx, &ln);
    if (stream_bytes) *stream_bytes = ctx->reads.len;
    if (records) *records = ln;
    return rc;
}

int dskgpu_push_raw(dskgpu_ctx* ctx, const char* text, uint64_t nbytes, int format, int new_file) {
    if (!ctx || (!text && nbytes) || (format != DSKGPU_RAW_FASTA && format != DSKGPU_RAW_FASTQ)) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    ReadStream& r = ctx->reads;
    if (!r.raw_pending) {
        CK(r.raw_state.ensure(sizeof(RawState)));
        CK(r.raw_in.ensure(PIN_CHUNK));
        const u64 maxb = PIN_CHUNK / RP_BLOCK;
        CK(r.raw_blk.ensure(maxb * sizeof(RpBlock)));
        CK(r.raw_boff.ensure(maxb * 8));
        CK(r.raw_bstate.ensure((maxb + 1) * 4));
        r.raw_base = r.raw_ub = r.len;
        hipLaunchKernelGGL(k_rp_init, dim3(1), dim3(1), 0, ctx->stream, r.raw_state.as<RawState>(), (unsigned long long)r.len);
        CKL("k_rp_init");
        r.raw_pending = true;
    } else if (new_file) {
        hipLaunchKernelGGL(k_rp_fresh, dim3(1), dim3(1), 0, ctx->stream, r.raw_state.as<RawState>());
        CKL("k_rp_fresh");
    }
    // what the text can leave at most: every byte, the separator in front of a new file, the terminator
    { const int e = stream_hold(ctx, r.raw_ub + nbytes + 2, r.raw_ub, true); if (e) return e; }
    uint8_t* out = r.own.as<uint8_t>();
    size_t len = 0;
    for (u64 off = 0; off < nbytes; off += len) {      // (one device buffer takes every piece: the stream orders the next piece's DMA behind this piece's kernels, which take a fraction of the DMA's time)
        { const int e = stage_piece(ctx, text + off, nbytes - off, r.raw_in.as<uint8_t>(), &len); if (e) return e; }
        if (format == DSKGPU_RAW_FASTQ) launch_raw_chunk<RP_FASTQ>(ctx, (u32)len, out);
        else launch_raw_chunk<RP_FASTA>(ctx, (u32)len, out);
        CKL("k_rp_write");
    }
    r.raw_ub += nbytes + 1;
    return DSKGPU_OK;
}

int dskgpu_stream_bytes(dskgpu_ctx* ctx, uint64_t* stream_bytes) {
    if (!ctx || !stream_bytes) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    *stream_bytes = ctx->reads.len;
    return DSKGPU_OK;
}

int dskgpu_rewind_reads(dskgpu_ctx* ctx, uint64_t stream_bytes) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    ReadStream& r = ctx->reads;
    if (ctx->enc_keep) return fail(ctx, DSKGPU_E_STATE, "dskgpu_rewind_reads: the reads were encoded and released (dskgpu_encode_reads)");
    if (stream_bytes > r.len) return fail(ctx, DSKGPU_E_ARG, "dskgpu_rewind_reads: the stream is shorter than that");
    r.len = stream_bytes;
    ctx->banks.cut_ends(stream_bytes);
    ctx->d_reads = r.own.as<uint8_t>(); ctx->n_bytes = r.len; ctx->reads_changed();
    return DSKGPU_OK;
}

int dskgpu_reserve_reads(dskgpu_ctx* ctx, uint64_t nbytes) {
    if (!ctx) return DSKGPU_E_ARG;
    CK(hipSetDevice(ctx->cfg.device));
    RAW_SYNC(ctx);
    ReadStream& r = ctx->reads;
    { const int e = ensure_pinned(ctx); if (e) return e; }
    if (nbytes + 1 <= r.own.cap) return DSKGPU_OK;      // (stream_hold would do nothing either; the return keeps d_reads from being re-pointed when nothing grew)
    { const int e = stream_hold(ctx, nbytes + 1, r.len, false); if (e) return e; }
    if (r.len) ctx->d_reads = r.own.as<uint8_t>();
    return DSKGPU_OK;
}

int dskgpu_set_reads_device(dskgpu_ctx* ctx, const void* d_bytes, uint64_t nbytes) {
    if (!ctx || (!d_bytes && nbytes)) return DSKGPU_E_ARG;
    // The caller usually just PRODUCED these bytes on a stream of its own (torch's), and the context's stream is non-blocking: nothing
    // orders the two.  Wait for the device once, here, so that a count can never read reads that are still being written (the r03
    // intermittent failure of the multi-process test was exactly that, in the test's reference count).  Once per read set, not per count.
    CK(hipSetDevice(ctx->cfg.device));
    CK(hipDeviceSynchronize());
    ctx->reads.raw_pending = false;
    ctx->d_reads = static_cast<const uint8_t*>(d_bytes); ctx->enc_keep = false; ctx->reads_changed();
    ctx->n_bytes = nbytes;
    ctx->reads.len = 0;
    ctx->banks.forget_ends();
    return DSKGPU_OK;
}
}  // extern "C"
