// bgzf_deflate.cpp -- include/ngsq_bgzf.h: host memory in, BGZF in host memory out, compressed on the device
// (bgzf_deflate.hip).
#include "../../include/ngsq_bgzf.h"

#include <cstdarg>
#include <cstring>

#include "context.h"
#include "device_out.h"

using namespace ngsq;

namespace {

int zfail(ngsq_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

} // namespace

namespace ngsq {
// the EOF block of the specification (SAM/BAM 4.1.2)
extern const uint8_t BGZF_EOF_BLOCK[28] = {0x1f, 0x8b, 0x08, 0x04, 0x00, 0x00, 0x00, 0x00, 0x00, 0xff, 0x06, 0x00, 0x42, 0x43,
                                           0x02, 0x00, 0x1b, 0x00, 0x03, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00, 0x00};
} // namespace ngsq

extern "C" {

uint64_t ngsq_bgzf_deflate_bound(uint64_t in_len, uint32_t flags) { return deflate_bound(in_len) + ((flags & NGSQ_BGZF_EOF) ? 28u : 0u); }

int ngsq_bgzf_set_effort(ngsq_ctx *c, uint32_t effort) {
    static_assert(NGSQ_BGZF_EFFORT_NORMAL == DEFLATE_EFFORT_NORMAL && NGSQ_BGZF_EFFORT_HIGH == DEFLATE_EFFORT_HIGH, "one numbering");
    if (!c) return zfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (effort > NGSQ_BGZF_EFFORT_HIGH) return zfail(c, NGSQ_ERR_INVALID_ARGUMENT, "unknown effort %u (0: normal, 1: high)", effort);
    c->bgzf_effort = effort;
    return NGSQ_OK;
}

uint32_t ngsq_bgzf_effort(const ngsq_ctx *c) { return c ? c->bgzf_effort : NGSQ_BGZF_EFFORT_NORMAL; }

uint32_t ngsq_bgzf_effort_candidates(uint32_t effort) {
    return effort == NGSQ_BGZF_EFFORT_NORMAL ? 1u : effort == NGSQ_BGZF_EFFORT_HIGH ? DEFLATE_CHAIN_K : 0u;
}

int ngsq_bgzf_deflate_device(ngsq_ctx *c, const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint32_t flags,
                             ngsq_bgzf_deflate_report *rep) {
    if (rep) memset(rep, 0, sizeof *rep);
    if (!c || !out_len || (in_len && !in) || (out_cap && !out)) return zfail(c, NGSQ_ERR_INVALID_ARGUMENT, "null argument");
    if (flags & ~NGSQ_BGZF_EOF) return zfail(c, NGSQ_ERR_INVALID_ARGUMENT, "unknown flags 0x%x", flags);
    const double t_begin = now_ms();
    const uint64_t eof = (flags & NGSQ_BGZF_EOF) ? sizeof BGZF_EOF_BLOCK : 0;
    *out_len = 0;
    uint64_t bytes = 0;
    if (in_len) {
        if (deflate_blocks(in_len) > 0x7FFFFFFFull) return zfail(c, NGSQ_ERR_LIMIT, "more than 2^31 blocks");
#define ZHIP(expr)                                                                                     \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return zfail(c, NGSQ_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
        hipStream_t st = c->stream;
        ZHIP(hipSetDevice(c->device));
        DevArray<uint8_t> d_in, d_out;
        DeflateScratch sc;
        MappedBuf hw;
        HipEvents<6> ev; // the encoder's four, and the brackets of the copies
        StreamDrain drain{st}; // (behind the arrays: it runs first)
        ZHIP(d_in.reserve(in_len + DEFLATE_IN_SLACK));
        ZHIP(d_out.reserve(deflate_bound(in_len)));
        ZHIP(hw.reserve(DEFLATE_HOST_WORDS * sizeof(unsigned long long)));
        memset(hw.h, 0, DEFLATE_HOST_WORDS * sizeof(unsigned long long));
        for (auto &x : ev.e) ZHIP(hipEventCreate(&x));
        ZHIP(hipEventRecord(ev.e[4], st));
        ZHIP(hipMemcpyAsync(d_in.p, in, in_len, hipMemcpyHostToDevice, st));
        ZHIP(hipMemsetAsync(d_in.p + in_len, 0, DEFLATE_IN_SLACK, st));
        ZHIP(launch_bgzf_deflate(d_in.p, in_len, d_out.p, sc, static_cast<unsigned long long *>(hw.dev), c->bgzf_effort, st, ev.e));
        ZHIP(hipStreamSynchronize(st));
        const unsigned long long *const h = static_cast<const unsigned long long *>(hw.h);
        bytes = h[DH_BYTES];
        float ms = 0, copy_ms = 0;
        if (hipEventElapsedTime(&ms, ev.e[4], ev.e[0]) == hipSuccess) copy_ms += ms;
        if (rep) {
            rep->blocks = deflate_blocks(in_len);
            rep->stored_blocks = h[DH_STORED];
            rep->tokens = h[DH_TOKENS];
            rep->matches = h[DH_MATCHES];
            if (hipEventElapsedTime(&ms, ev.e[0], ev.e[1]) == hipSuccess) rep->deflate_ms = ms;
            if (hipEventElapsedTime(&ms, ev.e[1], ev.e[2]) == hipSuccess) rep->crc_ms = ms;
            if (hipEventElapsedTime(&ms, ev.e[2], ev.e[3]) == hipSuccess) rep->pack_ms = ms;
        }
        if (bytes > deflate_bound(in_len)) return zfail(c, NGSQ_ERR_STATE, "the encoder wrote %llu bytes, more than its bound", (unsigned long long)bytes);
        *out_len = bytes + eof;
        if (bytes + eof <= out_cap) {
            ZHIP(hipEventRecord(ev.e[4], st));
            ZHIP(hipMemcpyAsync(out, d_out.p, bytes, hipMemcpyDeviceToHost, st));
            ZHIP(hipEventRecord(ev.e[5], st));
            ZHIP(hipStreamSynchronize(st));
            if (hipEventElapsedTime(&ms, ev.e[4], ev.e[5]) == hipSuccess) copy_ms += ms;
        }
        if (rep) rep->copy_ms = copy_ms;
#undef ZHIP
    }
    *out_len = bytes + eof;
    if (rep) {
        rep->in_bytes = in_len;
        rep->out_bytes = bytes + eof;
        rep->total_ms = now_ms() - t_begin;
    }
    if (bytes + eof > out_cap)
        return zfail(c, NGSQ_ERR_LIMIT, "output buffer too small: %llu > %llu", (unsigned long long)(bytes + eof), (unsigned long long)out_cap);
    if (eof) memcpy(out + bytes, BGZF_EOF_BLOCK, sizeof BGZF_EOF_BLOCK);
    return NGSQ_OK;
}

} // extern "C"
