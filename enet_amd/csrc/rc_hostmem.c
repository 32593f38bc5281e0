/*
 * rc_hostmem.c -- batches in host memory (enet_rc_*_batch_host).
 *
 * The arrays [in | in_off | in_len | out_off | out_cap | out_len | out] are
 * laid out in one pinned staging buffer and its device twin (struct
 * host_plan): the input goes up, the device path runs (rc_host.c run_device),
 * and only the produced bytes come back.  Caller memory is DMA'd or mapped
 * directly only where the caller page-locked it; pageable memory goes through
 * the pinned staging on the copy threads (rc_hostcopy.c).  Nothing here
 * page-locks or unlocks memory.
 */
#define _POSIX_C_SOURCE 200809L
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <time.h>

#include "rc_host_internal.h"   /* enet_rc_amd.h, rc_abi_internal.h, rc_ctx */

#define FAIL(err) rc_fail((int) (err), "rc_hostmem.c", __LINE__)
#define BIG_COPY (16u << 20)        /* copies in four overlapped groups; the GPU gather and slot copy */

/* The caller's arrays of one batch (or of one piece of a split batch). */
struct host_batch {
    int decompress;
    const uint8_t *in; const uint64_t *in_off; const uint32_t *in_len; size_t n;
    uint8_t *out; const uint64_t *out_off; const uint32_t *out_cap; uint32_t *out_len;
    int allow_pin;                  /* caller memory the caller page-locked may be DMA'd directly */
    /* the input is packet i's gather list gbuf[gfirst[i] .. gfirst[i + 1]),
       flattened into the staging; in_len = the flattened lengths */
    const ENetBuffer *gbuf; const size_t *gfirst;
};

struct host_plan {
    /* from the scan of the arrays */
    uint64_t in_bytes, out_bytes, in_lo;
    uint32_t max_len, max_cap;
    int packed_in;                  /* the input is one back-to-back range from in_lo */
    /* the input route: exactly one of pin_in, pitch, zc_dev, or none (staging) */
    int pin_in;                     /* one DMA straight from the caller's range */
    uint64_t pitch, row;            /* strided DMA: slots pitch apart, rows row apart on the device */
    const uint8_t *zc_dev;          /* GPU gather: the caller's mapped range from in + zc_lo */
    uint64_t zc_lo;
    uint64_t dev_in;                /* device input bytes: back to back, or (GPU gather) granule-padded */
    /* staging layout (offsets in h_stage and d_stage) */
    size_t a_in, a_ioff, a_ilen, a_ooff, a_ocap, a_olen, a_out, a_soff, total;
    double tp[6];                   /* ENET_RC_HOST_PROFILE stamps */
};

static double now_ms(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return t.tv_sec * 1e3 + t.tv_nsec * 1e-6;
}

/* ENET_RC_HOST_PROFILE=1: the phase times of a host batch on stderr (tp[4]:
 * the pack route's stamp between its packing and its D2H) */
static void profile_line(const struct host_batch *b, const struct host_plan *p, const char *route, double out_mb)
{
    if (!rc_host_cfg()->profile) return;
    const double *tp = p->tp, end = now_ms(), mid = tp[4] > 0 ? tp[4] : tp[3];
    fprintf(stderr, "enet_rc host %s n=%zu in=%.1f MB out=%.1f MB (%s): stage+H2D enqueue %.3f, H2D drain %.3f, "
            "kernels %.3f, pack+lens %.3f, results %.3f, total %.3f ms\n", b->decompress ? "dec" : "enc", b->n,
            p->in_bytes / 1e6, out_mb, route, tp[1] - tp[0], tp[2] - tp[1], tp[3] - tp[2], mid - tp[3], end - mid,
            end - tp[0]);
}

/* 1: [p, p + bytes) may be DMA'd or mapped directly: the caller page-locked
 * it (its own hipHostMalloc or registration, e.g. a long-lived receive
 * buffer) and the whole range lies inside that one allocation or
 * registration.  0: pageable memory, a range that only touches memory some
 * other caller registered (whose registration may end during our transfer),
 * a range below 1 MiB, or ENET_RC_NO_HOST_PIN -- the pinned staging then. */
static int caller_pinned(const void *p, size_t bytes)
{
    if (rc_host_cfg()->no_pin || bytes < (1u << 20)) return 0;
    hipPointerAttribute_t at;
    void *start = NULL;
    size_t size = 0;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost &&
        hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t) p) == hipSuccess &&
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t) p) == hipSuccess &&
        (uintptr_t) p >= (uintptr_t) start && (uintptr_t) p + bytes <= (uintptr_t) start + size)
        return 1;
    (void) hipGetLastError();
    return 0;
}

/* A host-to-device copy from page-locked memory as 2D copies (rows of 1 MiB,
 * or 64 KiB below 4 MiB; the tail as two overlapping rows): the runtime runs
 * 2D copies on a DMA engine, a plain one of this size as a copy kernel, which
 * takes CUs from the kernels of the pieces already running (run_host_split).
 * ENET_RC_H2D_DMA=0: plain copies. */
static hipError_t h2d_copy(void *dst, const void *src, size_t bytes, hipStream_t s)
{
    const size_t w = bytes >= (4u << 20) ? (1u << 20) : (1u << 16), rows = bytes / w;
    /* (past 48 MB the runtime ran some 2D copies as a row-by-row copy kernel
     * at a tenth of the link's rate: C4's pieces, profiles/r5s_split) */
    if (!rc_host_cfg()->h2d_dma || rows < 2 || bytes > (48u << 20))
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s);
    hipError_t err = hipMemcpy2DAsync(dst, w, src, w, w, rows, hipMemcpyHostToDevice, s);
    const size_t t = bytes - rows * w;
    if (err == hipSuccess && t) {
        /* the last 2 * ceil(t / 2) bytes (re-copying at most one byte of the rows) */
        const size_t h = (t + 1) / 2, at = bytes - 2 * h;
        err = hipMemcpy2DAsync((uint8_t *) dst + at, h, (const uint8_t *) src + at, h, h, 2, hipMemcpyHostToDevice, s);
    }
    return err;
}

/* ------------------------------------------------------------ 1. the plan */
/* The input as it goes to the device: packed back to back (a batch whose
 * packets sit in gapped slots -- the compressed side of a round trip -- moves
 * only its bytes); a batch that already is back to back is one range. */
static void plan_scan(struct host_plan *p, const struct host_batch *b)
{
    p->in_lo = b->gbuf ? 0 : b->in_off[0];
    p->packed_in = b->gbuf == NULL;
    for (size_t i = 0; i < b->n; ++i) {
        if (!b->gbuf && b->in_off[i] != p->in_lo + p->in_bytes) p->packed_in = 0;
        p->in_bytes += b->in_len[i];
        const uint64_t f = b->out_off[i] + b->out_cap[i];
        if (f > p->out_bytes) p->out_bytes = f;
        if (b->in_len[i] > p->max_len) p->max_len = b->in_len[i];
        if (b->out_cap[i] > p->max_cap) p->max_cap = b->out_cap[i];
    }
}

/* An input in gapped slots in memory the caller page-locked
 * (ENET_RC_GPU_COPY=0: through pinned staging on the host instead):
 *  - slots at a uniform pitch (a caller's array of fixed-size buffers): one
 *    strided DMA (hipMemcpy2DAsync: max_len bytes of each slot, rows
 *    round_up(max_len, 16) apart on the device);
 *  - other gaps: the buffer is mapped and rc_gather16 (rc_pack.hip) reads the
 *    packets over PCIe in whole 16-B granules into the device input (each
 *    packet in granules of its own, at its source alignment), so the gaps
 *    between slots never cross PCIe.
 * An input that is one range goes up in one DMA when the caller page-locked
 * it; everything else through the pinned staging. */
static void plan_route(struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n;
    const uint8_t *in = b->in;
    const uint64_t *in_off = b->in_off;
    const uint32_t *in_len = b->in_len;
    p->dev_in = p->in_bytes;
    if (!b->allow_pin || b->gbuf) return;
    if (p->packed_in) {
        p->pin_in = caller_pinned(in + p->in_lo, p->in_bytes);
        return;
    }
    if (!rc_host_cfg()->gpu_copy || p->in_bytes < BIG_COPY) return;
    if (n >= 2 && in_off[1] > in_off[0] && in_off[1] - in_off[0] >= p->max_len) {
        uint64_t pitch = in_off[1] - in_off[0];
        for (size_t i = 2; i < n && pitch; ++i)
            if (in_off[i] != in_off[0] + i * pitch) pitch = 0;
        if (pitch && caller_pinned(in + in_off[0], in_off[n - 1] + in_len[n - 1] - in_off[0])) {
            p->pitch = pitch;
            p->zc_lo = in_off[0];
            p->row = (p->max_len + 15) & ~(uint64_t) 15;
            p->dev_in = n * p->row;
            return;
        }
    }
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t i = 0; i < n; ++i)
        if (in_len[i]) {
            if (in_off[i] < lo) lo = in_off[i];
            if (in_off[i] + in_len[i] > hi) hi = in_off[i] + in_len[i];
        }
    void *dp = NULL;
    if (hi <= lo || !caller_pinned(in + lo, hi - lo)) return;
    /* (the mapping keeps the page offset: granule phases match) */
    if (hipHostGetDevicePointer(&dp, (void *) (in + lo), 0) != hipSuccess || !dp ||
        (((uintptr_t) dp ^ (uintptr_t) (in + lo)) & 4095) != 0) {
        (void) hipGetLastError();
        return;
    }
    p->zc_dev = (const uint8_t *) dp;
    p->zc_lo = lo;
    p->dev_in = 0;
    for (size_t i = 0; i < n; ++i)
        if (in_len[i]) p->dev_in += (((uintptr_t) (in + in_off[i]) & 15) + in_len[i] + 15) & ~(uint64_t) 15;
}

/* ---------------------------------------------- 2. the layout and reserve */
static int plan_layout(rc_ctx *c, struct host_plan *p, size_t n)
{
    p->a_in = 0;
    p->a_ioff = (p->a_in + p->dev_in + 15) & ~(size_t) 15;
    p->a_ilen = p->a_ioff + n * 8;
    p->a_ooff = (p->a_ilen + n * 4 + 15) & ~(size_t) 15;
    p->a_ocap = p->a_ooff + n * 8;
    p->a_olen = (p->a_ocap + n * 4 + 15) & ~(size_t) 15;
    p->a_out = (p->a_olen + n * 4 + 15) & ~(size_t) 15;
    p->total = p->a_out + p->out_bytes + 16;
    p->a_soff = (p->total + 15) & ~(size_t) 15;         /* source offsets of a device-side gather */
    if (stage_reserve(c, p->a_soff + n * 8) != 0 || pack_reserve(c, p->out_bytes + 16, (n + 1023) / 1024) != 0)
        return (int) hipErrorOutOfMemory;
    return 0;
}

/* ------------------------------------------------------------ 3. the upload */
/* each packet's offset in the device input, into the staging */
static void fill_dev_offsets(uint64_t *hio, const struct host_plan *p, const struct host_batch *b)
{
    uint64_t acc = 0;
    for (size_t i = 0; i < b->n; ++i) {
        const uint32_t l = b->in_len[i];
        if (p->pitch) {
            hio[i] = i * p->row;
        } else if (p->zc_dev) {
            const uint64_t ph = (uintptr_t) (b->in + b->in_off[i]) & 15;
            hio[i] = l ? acc + ph : acc;
            if (l) acc += (ph + l + 15) & ~(uint64_t) 15;
        } else {
            hio[i] = acc;
            acc += l;
        }
    }
}

/* the payload straight from memory the caller page-locked */
static hipError_t upload_direct(rc_ctx *c, const struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    if (p->pin_in) return h2d_copy(d + p->a_in, b->in + p->in_lo, p->in_bytes, c->stream);
    if (p->pitch) {
        hipError_t err = hipMemcpy2DAsync(d + p->a_in, p->row, b->in + p->zc_lo, p->pitch, p->max_len, n - 1,
                                          hipMemcpyHostToDevice, c->stream);
        if (err == hipSuccess && b->in_len[n - 1])
            err = hipMemcpyAsync(d + p->a_in + (n - 1) * p->row, b->in + b->in_off[n - 1], b->in_len[n - 1],
                                 hipMemcpyHostToDevice, c->stream);
        return err;
    }
    uint64_t *hso = (uint64_t *) (h + p->a_soff);
    for (size_t i = 0; i < n; ++i) hso[i] = b->in_len[i] ? b->in_off[i] - p->zc_lo : 0;
    hipError_t err = hipMemcpyAsync(d + p->a_soff, h + p->a_soff, n * 8, hipMemcpyHostToDevice, c->stream);
    if (err != hipSuccess) return err;
    return (hipError_t) rc_hip_gather16(p->zc_dev, (const uint64_t *) (d + p->a_soff), d + p->a_in,
                                        (const uint64_t *) (d + p->a_ioff), (const uint32_t *) (d + p->a_ilen),
                                        (uint32_t) n, (void *) c->stream);
}

/* the payload in four packet groups through pinned staging, the staging copy
 * of group k+1 overlapping the DMA of group k */
static hipError_t upload_staged(rc_ctx *c, const struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    const uint64_t *hio = (const uint64_t *) (h + p->a_ioff);
    const size_t ig = p->in_bytes >= BIG_COPY ? 4 : 1;
    for (size_t g = 0; g < ig; ++g) {
        const size_t lo = n * g / ig, hi = n * (g + 1) / ig;
        if (hi <= lo) continue;
        const uint64_t b0 = hio[lo], b1 = hio[hi - 1] + b->in_len[hi - 1];
        if (b->gbuf) rc_par_gather(h + p->a_in, hio, b->gbuf, b->gfirst, lo, hi, b1 - b0);
        else if (p->packed_in) rc_par_memcpy(h + p->a_in + b0, b->in + p->in_lo + b0, b1 - b0);
        else rc_par_scatter(h + p->a_in, hio, b->in, b->in_off, b->in_len, lo, hi, b1 - b0);
        if (b1 == b0) continue;
        hipError_t err = hipMemcpyAsync(d + p->a_in + b0, h + p->a_in + b0, b1 - b0, hipMemcpyHostToDevice, c->stream);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

static void h2d_sync_set(struct h2d_sync *y, int v)
{
    pthread_mutex_lock(&y->m);
    if (!y->ready) y->ready = v;
    pthread_cond_broadcast(&y->cv);
    pthread_mutex_unlock(&y->m);
}

/* Enqueues the arrays and the payload; a piece of a split batch after the
 * previous piece's input DMA, and signalling the next piece. */
static int upload(rc_ctx *c, const struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    fill_dev_offsets((uint64_t *) (h + p->a_ioff), p, b);
    memcpy(h + p->a_ilen, b->in_len, n * 4);
    memcpy(h + p->a_ooff, b->out_off, n * 8);
    memcpy(h + p->a_ocap, b->out_cap, n * 4);
    if (c->sync_wait) {             /* a later piece: its DMA after the previous piece's */
        struct h2d_sync *y = c->sync_wait;
        pthread_mutex_lock(&y->m);
        while (!y->ready) pthread_cond_wait(&y->cv, &y->m);
        const int r = y->ready;
        pthread_mutex_unlock(&y->m);
        if (r > 0) (void) hipStreamWaitEvent(c->stream, y->ev, 0);
    }
    hipError_t err = h2d_copy(d + p->a_ioff, h + p->a_ioff, p->a_olen - p->a_ioff, c->stream);
    if (err != hipSuccess) return FAIL(err);
    const int direct = p->pin_in || p->pitch || p->zc_dev;
    err = direct ? upload_direct(c, p, b) : upload_staged(c, p, b);
    if (err != hipSuccess) {
        /* (a DMA or gather of the caller's memory may be in flight, and the
         * caller may free that memory once the call has returned) */
        if (direct) hipStreamSynchronize(c->stream);
        return FAIL(err);
    }
    c->last_paths = p->zc_dev ? 4u : p->pitch ? 3u : p->pin_in ? 2u : 1u;
    if (c->sync_sig)                /* its input DMA is enqueued: the next piece's may follow */
        h2d_sync_set(c->sync_sig, hipEventRecord(c->sync_sig->ev, c->stream) == hipSuccess ? 1 : -1);
    return 0;
}

/* ----------------------------------------------------------- 4. the results
 * Each route either handles the batch (0, or a HIP error) or says NOT_MINE;
 * on success the stream has drained. */
#define NOT_MINE (-1)

/* the exact-path count behind a results copy into caller memory; drains the
 * stream even when an enqueue failed (the copy may be writing that memory, and
 * the caller may free it once the call has returned) */
static hipError_t results_drain(rc_ctx *c, hipError_t err)
{
    if (err == hipSuccess) err = hipMemcpyAsync(&c->last_exact, c->ws.counters, 4, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    return err == hipSuccess ? e2 : err;
}

/* small batches (the per-datagram drop-in calls): one D2H of the slots, fewer
 * launches and syncs than packing */
static int results_small(rc_ctx *c, const struct host_plan *p, const struct host_batch *b)
{
    uint8_t *h = c->h_stage, *d = c->d_stage;
    if (p->out_bytes > (1u << 20)) return NOT_MINE;
    hipError_t err = hipMemcpyAsync(h + p->a_olen, d + p->a_olen, p->total - 16 - p->a_olen, hipMemcpyDeviceToHost,
                                    c->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(&c->last_exact, c->ws.counters, 4, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) return FAIL(err);
    memcpy(b->out_len, h + p->a_olen, b->n * 4);
    for (size_t i = 0; i < b->n; ++i)
        if (b->out_len[i]) memcpy(b->out + b->out_off[i], h + p->a_out + b->out_off[i], b->out_len[i]);
    c->last_paths |= 1u << 4;
    return 0;
}

/* A decompress batch whose slots are back to back (out_cap = the packet
 * lengths) and every one of them filled, into memory the caller page-locked:
 * the whole span in one DMA straight behind the kernels.  The lengths are
 * read first: a slot a packet did not fill (a corrupt stream, an output that
 * does not fit) keeps the caller's bytes past its out_len, as compress.c
 * writes only what it decodes -- the span's DMA would put the staging
 * memory's old contents there (an earlier batch's payload) -- so such a batch
 * is not this route's. */
static int results_span(rc_ctx *c, const struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    int contig = b->decompress && rc_host_cfg()->contig_dma;
    for (size_t i = 1; i < n && contig; ++i) contig = b->out_off[i] == b->out_off[i - 1] + b->out_cap[i - 1];
    if (!contig) return NOT_MINE;
    hipError_t err = hipMemcpyAsync(h + p->a_olen, d + p->a_olen, n * 4, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) return FAIL(err);
    const uint32_t *ol = (const uint32_t *) (h + p->a_olen);
    for (size_t i = 0; i < n && contig; ++i) contig = ol[i] == b->out_cap[i];
    const uint64_t span = b->out_off[n - 1] + b->out_cap[n - 1] - b->out_off[0];
    if (!contig || !b->allow_pin || !caller_pinned(b->out + b->out_off[0], span)) return NOT_MINE;
    err = hipMemcpyAsync(b->out + b->out_off[0], d + p->a_out + b->out_off[0], span, hipMemcpyDeviceToHost, c->stream);
    err = results_drain(c, err);
    if (err != hipSuccess) return FAIL(err);
    memcpy(b->out_len, ol, n * 4);
    profile_line(b, p, "direct", span / 1e6);
    c->last_paths |= 2u << 4;
    return 0;
}

/* The results straight from their device slots into the caller's slots by
 * the GPU (rc_slot_copy writing the mapped caller buffer, which the caller
 * page-locked, over PCIe): no packing pass and no host scatter.
 * ENET_RC_GPU_COPY=0: packed on the device, D2H and scattered on the host. */
static int results_slot_copy(rc_ctx *c, const struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n;
    uint8_t *d = c->d_stage;
    if (!b->allow_pin || !rc_host_cfg()->gpu_copy || p->out_bytes < BIG_COPY) return NOT_MINE;
    uint64_t lo = UINT64_MAX, hi = 0;
    for (size_t i = 0; i < n; ++i) {
        if (b->out_off[i] < lo) lo = b->out_off[i];
        if (b->out_off[i] + b->out_cap[i] > hi) hi = b->out_off[i] + b->out_cap[i];
    }
    void *dp = NULL;
    if (hi <= lo || !caller_pinned(b->out + lo, hi - lo)) return NOT_MINE;
    if (hipHostGetDevicePointer(&dp, (void *) (b->out + lo), 0) != hipSuccess || !dp) {
        (void) hipGetLastError();
        return NOT_MINE;
    }
    /* (a piece of a split batch of packets of >= 512 B on average: its slot
     * copy with few workgroups, leaving the other pieces' kernels their CUs'
     * issue slots; the copy's wavefronts each move a packet, so smaller
     * packets need them all to keep PCIe busy) */
    const uint32_t wgs = (c->sync_sig || c->sync_wait) && p->in_bytes >= 512 * (uint64_t) n
                             ? rc_host_cfg()->piece_copy_wgs : 0u;
    uint8_t *h = c->h_stage;
    hipError_t err = (hipError_t) rc_hip_slot_copy(d + p->a_out, (const uint64_t *) (d + p->a_ooff),
                                                   (const uint32_t *) (d + p->a_olen), (uint32_t) n,
                                                   (uint8_t *) dp - lo, wgs, (void *) c->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(h + p->a_olen, d + p->a_olen, n * 4, hipMemcpyDeviceToHost, c->stream);
    err = results_drain(c, err);
    if (err != hipSuccess) return FAIL(err);
    memcpy(b->out_len, h + p->a_olen, n * 4);
    profile_line(b, p, "GPU slot copy", p->out_bytes / 1e6);
    c->last_paths |= 3u << 4;
    return 0;
}

/* packed's bytes (poff[i]: packet i's offset in them) from the device in
 * packet groups into the staging, the scatter of group g to the caller's
 * slots overlapping the DMA of g+1 */
static hipError_t d2h_scatter(rc_ctx *c, const struct host_plan *p, const struct host_batch *b, const uint64_t *poff,
                              uint64_t packed)
{
    const size_t n = b->n, groups = packed >= BIG_COPY ? 4 : 1;
    uint8_t *h = c->h_stage;
    hipError_t err = hipSuccess;
    hipEvent_t ev[4];
    size_t nev = 0, first[5];
    for (size_t g = 0; g <= groups; ++g) first[g] = n * g / groups;
    for (size_t g = 0; g < groups && err == hipSuccess; ++g) {
        const uint64_t lo = poff[first[g]], hi = poff[first[g + 1]];
        if (hi > lo) err = hipMemcpyAsync(h + p->a_out + lo, c->d_pack + lo, hi - lo, hipMemcpyDeviceToHost, c->stream);
        if (err == hipSuccess) err = hipEventCreateWithFlags(&ev[g], hipEventDisableTiming);
        if (err == hipSuccess) { nev = g + 1; err = hipEventRecord(ev[g], c->stream); }
    }
    for (size_t g = 0; g < nev && err == hipSuccess; ++g) {
        err = hipEventSynchronize(ev[g]);
        if (err == hipSuccess)
            rc_par_scatter(b->out, b->out_off, h + p->a_out, poff, b->out_len, first[g], first[g + 1],
                           poff[first[g + 1]] - poff[first[g]]);
    }
    for (size_t g = 0; g < nev; ++g) hipEventDestroy(ev[g]);
    return err;
}

/* the results packed back to back on the device (rc_pack.hip), so that only
 * the produced bytes cross PCIe, and scattered to out_off on the host */
static int results_pack(rc_ctx *c, struct host_plan *p, const struct host_batch *b)
{
    const size_t n = b->n, blocks = (n + 1023) / 1024;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    const int rc = rc_hip_pack(d + p->a_out, (const uint64_t *) (d + p->a_ooff), (const uint32_t *) (d + p->a_olen),
                               (uint32_t) n, c->d_bsum, c->d_pack, (void *) c->stream);
    if (rc != 0) return FAIL(rc);
    uint64_t packed = 0;
    hipError_t err = hipMemcpyAsync(h + p->a_olen, d + p->a_olen, n * 4, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(&c->last_exact, c->ws.counters, 4, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipMemcpyAsync(&packed, c->d_bsum + blocks, 8, hipMemcpyDeviceToHost, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) return FAIL(err);
    if (rc_host_cfg()->profile) p->tp[4] = now_ms();
    if (packed > p->out_bytes) return FAIL(hipErrorUnknown);
    memcpy(b->out_len, h + p->a_olen, n * 4);
    uint64_t *poff = (uint64_t *) malloc((n + 1) * sizeof(uint64_t));
    if (!poff) return FAIL(hipErrorOutOfMemory);
    uint64_t acc = 0;
    for (size_t i = 0; i < n; ++i) { poff[i] = acc; acc += b->out_len[i]; }
    poff[n] = acc;
    err = d2h_scatter(c, p, b, poff, packed);
    free(poff);
    profile_line(b, p, "pack", packed / 1e6);
    c->last_paths |= 4u << 4;
    return err == hipSuccess ? 0 : FAIL(err);
}

/* One batch (or one piece) on one context. */
static int run_host(rc_ctx *c, const struct host_batch *b)
{
    const int prof = rc_host_cfg()->profile;
    struct host_plan p = {0};
    if (prof) p.tp[0] = now_ms();
    if (!c) return (int) hipErrorInvalidValue;
    if (b->n == 0) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return (int) hipErrorInvalidDevice;
    plan_scan(&p, b);
    plan_route(&p, b);
    int rc = plan_layout(c, &p, b->n);
    if (rc != 0) return FAIL(rc);
    rc = upload(c, &p, b);
    if (rc != 0) return rc;
    if (prof) { p.tp[1] = now_ms(); hipStreamSynchronize(c->stream); p.tp[2] = now_ms(); }
    uint8_t *d = c->d_stage;
    rc = run_device(c, b->decompress, d + p.a_in, (const uint64_t *) (d + p.a_ioff), (const uint32_t *) (d + p.a_ilen),
                    b->n, p.max_len, p.max_cap, d + p.a_out, (const uint64_t *) (d + p.a_ooff),
                    (const uint32_t *) (d + p.a_ocap), (uint32_t *) (d + p.a_olen), (void *) c->stream);
    if (rc != 0) return FAIL(rc);
    if (prof) { hipStreamSynchronize(c->stream); p.tp[3] = now_ms(); }
    rc = results_small(c, &p, b);
    if (rc == NOT_MINE) rc = results_span(c, &p, b);
    if (rc == NOT_MINE) rc = results_slot_copy(c, &p, b);
    if (rc == NOT_MINE) rc = results_pack(c, &p, b);
    return rc;
}

/* ---- a large host batch in pieces, on this context and further contexts
 * on the same device (each with its own stream and workspace): each piece's
 * input DMA follows the previous piece's, so its kernels start while the
 * later pieces' inputs still cross PCIe and run beside the earlier pieces'
 * on the other CUs, and the earlier pieces' results cross PCIe while the later
 * ones compute.  The lane kernels take as long for part of a batch as for the
 * whole (a packet per lane), so the pieces run side by side,
 * never one after the other.  Pieces hold equal input bytes.  Pieces of
 * pageable caller memory take each piece's pinned staging: their host copies
 * then run on the pieces' threads side by side.  ENET_RC_HOST_SPLIT=k: k
 * pieces (2..SPLIT_MAX; 0 or 1: off). */
typedef struct {
    rc_ctx *c;
    struct host_batch b;
    uint64_t *rebased;              /* the piece's out_off from its own first slot */
    pthread_t th;
    int threaded, rc;
} piece_job;

static void *piece_worker(void *p)
{
    piece_job *j = (piece_job *) p;
    j->rc = run_host(j->c, &j->b);
    /* (a failed piece may have left DMAs of the caller's memory in flight,
     * and the caller may free that memory once the call has returned) */
    if (j->rc != 0) hipStreamSynchronize(j->c->stream);
    /* (a piece that ended before its input DMA: the next one waits for nothing) */
    if (j->c->sync_sig) h2d_sync_set(j->c->sync_sig, -1);
    return NULL;
}

#define SPLIT_MIN_PACKETS 8192u         /* per piece */
#define SPLIT_MIN_BYTES (8ull << 20)    /* per piece */

/* The pieces of a batch: 1, or 2..split_k with a context for each */
static int split_count(rc_ctx *c, const struct host_batch *b, uint64_t *bytes)
{
    const size_t n = b->n;
    int k = c->split_k;
    uint64_t ilo = UINT64_MAX, ihi = 0, olo = UINT64_MAX, ohi = 0;
    *bytes = 0;
    if (k < 2 || n < 32768 || c->ws.kernel == RC_KERNEL_WAVE) return 1;
    for (size_t i = 0; i < n; ++i) {
        *bytes += b->in_len[i];
        if (b->in_len[i]) {
            if (b->in_off[i] < ilo) ilo = b->in_off[i];
            if (b->in_off[i] + b->in_len[i] > ihi) ihi = b->in_off[i] + b->in_len[i];
        }
        if (b->out_off[i] < olo) olo = b->out_off[i];
        if (b->out_off[i] + b->out_cap[i] > ohi) ohi = b->out_off[i] + b->out_cap[i];
    }
    if (*bytes < (32ull << 20)) return 1;           /* (smaller batches: one piece) */
    while (k > 1 && (n < (size_t) k * SPLIT_MIN_PACKETS || *bytes < (uint64_t) k * SPLIT_MIN_BYTES)) --k;
    if (k < 2 || ihi <= ilo || ohi <= olo) return 1;
    if (hipSetDevice(c->device) != hipSuccess) return 1;
    for (int i = 0; i < k - 1; ++i)
        if (!c->twin[i]) {
            c->twin[i] = enet_range_coder_create();
            if (!c->twin[i]) return i + 1;
            ctx_copy_config((rc_ctx *) c->twin[i], c);
        }
    return k;
}

/* piece boundaries at equal shares of the input bytes */
static void split_bounds(size_t *first, int k, const uint32_t *in_len, size_t n, uint64_t bytes)
{
    uint64_t acc = 0;
    size_t i = 0;
    first[0] = 0;
    first[k] = n;
    for (int p = 1; p < k; ++p) {
        const uint64_t goal = bytes * (uint64_t) p / (uint64_t) k;
        while (i < n && acc + in_len[i] <= goal) acc += in_len[i++];
        /* whole 2048-packet groups: a piece's decoder and code-pass
           workgroups (256 packets each) then spread evenly over the 8
           XCDs, and the pieces' workgroups together fill each XCD's CUs
           once (a piece one workgroup over lands it on a busy CU and
           doubles that piece's time) */
        size_t f = (i + 1024) & ~(size_t) 2047;
        if (f <= first[p - 1]) f = first[p - 1] + 2048;
        first[p] = f < n ? f : n;
    }
}

/* piece p of k: packets [a, a + m) of b on context x */
static void piece_init(piece_job *j, rc_ctx *x, const struct host_batch *b, size_t a, size_t m)
{
    /* the piece's output offsets from its own first slot, so that its
     * staging (sized from the largest out_off + out_cap) covers its slots
     * only, not the output from byte 0 */
    uint64_t lo = UINT64_MAX;
    for (size_t i = a; i < a + m; ++i) if (b->out_off[i] < lo) lo = b->out_off[i];
    j->c = x;
    j->rc = j->threaded = 0;
    j->rebased = m ? (uint64_t *) malloc(m * sizeof(uint64_t)) : NULL;
    for (size_t i = 0; i < m && j->rebased; ++i) j->rebased[i] = b->out_off[a + i] - lo;
    j->b = *b;
    j->b.in_off += a; j->b.in_len += a; j->b.out_cap += a; j->b.out_len += a;
    j->b.n = m;
    j->b.out = j->rebased ? b->out + lo : b->out;
    j->b.out_off = j->rebased ? j->rebased : b->out_off + a;
}

static int sync_init(struct h2d_sync *y)
{
    if (hipEventCreateWithFlags(&y->ev, hipEventDisableTiming) != hipSuccess) return -1;
    pthread_mutex_init(&y->m, NULL);
    pthread_cond_init(&y->cv, NULL);
    y->ready = 0;
    return 0;
}

static void sync_destroy(struct h2d_sync *y, int n)
{
    for (int i = 0; i < n; ++i) {
        hipEventDestroy(y[i].ev);
        pthread_cond_destroy(&y[i].cv);
        pthread_mutex_destroy(&y[i].m);
    }
}

static int run_host_split(rc_ctx *c, const struct host_batch *b)
{
    if (!c) return (int) hipErrorInvalidValue;
    c->last_split = 0;
    uint64_t bytes = 0;
    const int k = split_count(c, b, &bytes);
    struct h2d_sync y[SPLIT_MAX - 1];
    int ny = 0;
    while (ny < k - 1 && sync_init(&y[ny]) == 0) ++ny;
    if (k < 2 || ny < k - 1) {      /* (no further context or event: one piece) */
        sync_destroy(y, ny);
        return run_host(c, b);
    }
    size_t first[SPLIT_MAX + 1];
    split_bounds(first, k, b->in_len, b->n, bytes);
    piece_job job[SPLIT_MAX];
    for (int p = 0; p < k; ++p) {
        rc_ctx *x = p ? (rc_ctx *) c->twin[p - 1] : c;
        piece_init(&job[p], x, b, first[p], first[p + 1] - first[p]);
        x->sync_wait = p ? &y[p - 1] : NULL;
        x->sync_sig = p < k - 1 ? &y[p] : NULL;
    }
    for (int p = 1; p < k; ++p) job[p].threaded = pthread_create(&job[p].th, NULL, piece_worker, &job[p]) == 0;
    piece_worker(&job[0]);
    for (int p = 1; p < k; ++p) {
        if (job[p].threaded) pthread_join(job[p].th, NULL);
        else piece_worker(&job[p]);     /* (its predecessors have all signalled by now) */
    }
    int rc = 0;
    uint32_t exact = 0;
    for (int p = 0; p < k; ++p) {
        rc_ctx *x = job[p].c;
        x->sync_wait = x->sync_sig = NULL;
        if (!rc) rc = job[p].rc;
        exact += x->last_exact;
        free(job[p].rebased);
    }
    c->last_exact = exact;
    sync_destroy(y, k - 1);
    c->last_split = k;
    return rc;
}

int enet_rc_compress_batch_host(void *context, const uint8_t *in, const uint64_t *in_off,
                                const uint32_t *in_len, size_t n, uint8_t *out,
                                const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len)
{
    const struct host_batch b = {0, in, in_off, in_len, n, out, out_off, out_cap, out_len, 1, NULL, NULL};
    return run_host_split((rc_ctx *) context, &b);
}

int enet_rc_decompress_batch_host(void *context, const uint8_t *in, const uint64_t *in_off,
                                  const uint32_t *in_len, size_t n, uint8_t *out,
                                  const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len)
{
    const struct host_batch b = {1, in, in_off, in_len, n, out, out_off, out_cap, out_len, 1, NULL, NULL};
    return run_host_split((rc_ctx *) context, &b);
}

/* compress.c:246-342 over a batch of gather lists: packet i is
 * buffers[first[i] .. first[i + 1]), consumed as enet_range_coder_compress
 * consumes its inBuffers (protocol.c:1688-1695 passes &buffers[1],
 * bufferCount - 1); the lists are flattened straight into the pinned
 * staging on the copy threads. */
int enet_rc_compress_gather_batch_host(void *context, const ENetBuffer *buffers, const size_t *first, size_t n,
                                       uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                                       uint32_t *out_len)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c || (n && (!buffers || !first))) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    uint32_t *len = (uint32_t *) malloc(n * sizeof(uint32_t));
    if (!len) return (int) hipErrorOutOfMemory;
    for (size_t i = 0; i < n; ++i) {
        /* the lists must not run backwards: the copy threads flatten
           first[i + 1] - first[i] buffers of packet i */
        if (first[i + 1] < first[i]) { free(len); return (int) hipErrorInvalidValue; }
        const size_t l = rc_gather_len(buffers + first[i], first[i + 1] - first[i]);
        if (l > 0xFFFFFFFFu) { free(len); return (int) hipErrorInvalidValue; }
        len[i] = (uint32_t) l;
    }
    const struct host_batch b = {0, NULL, NULL, len, n, out, out_off, out_cap, out_len, 0, buffers, first};
    const int rc = run_host(c, &b);
    free(len);
    return rc;
}

/* for rc_multi.c: one device's share of a multi-device batch, always through
 * the pinned staging (the shares' ranges lie in one caller buffer) */
int rc_ctx_run_host(void *context, int decompress, const uint8_t *in, const uint64_t *in_off,
                    const uint32_t *in_len, size_t n, uint8_t *out, const uint64_t *out_off,
                    const uint32_t *out_cap, uint32_t *out_len)
{
    const struct host_batch b = {decompress, in, in_off, in_len, n, out, out_off, out_cap, out_len, 0, NULL, NULL};
    return run_host((rc_ctx *) context, &b);
}
