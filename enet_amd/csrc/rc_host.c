/*
 * rc_host.c -- C host side of the MI355X range coder.
 *
 * Implements the reference's compressor plugin surface (enet.h:323-335,
 * :574, :603-606) on top of the HIP kernels in rc_kernels.hip:
 *   - a coder context owns a HIP stream, a device workspace and pinned
 *     staging;
 *   - the per-datagram entry points run a one-packet batch on the GPU (the
 *     gather list is flattened on the host exactly as compress.c:275-284
 *     consumes it);
 *   - the batch entry points hand whole packet batches to the kernels
 *     (those that take host pointers are in rc_hostmem.c).
 * There is no CPU coder in this library: if no HIP device is usable,
 * enet_range_coder_create() returns NULL and the batch calls fail.
 */
#define _POSIX_C_SOURCE 200809L
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>

#include "rc_host_internal.h"   /* enet_rc_amd.h, rc_abi_internal.h, rc_ctx */

/* ENet's allocator and host hook, resolved from libenet when it is linked
 * (callbacks.c:37-52, host.c:294-304). */
extern void *enet_malloc(size_t) __attribute__((weak));
extern void enet_free(void *) __attribute__((weak));
extern void enet_host_compress(ENetHost *, const ENetCompressor *) __attribute__((weak));

#define SPLIT_DEFAULT 3
#define EXACT_SLOTS 256u            /* concurrent exact-path packets (64 KiB pool each) */

static void *ctx_alloc(size_t n) { return enet_malloc ? enet_malloc(n) : malloc(n); }
static void ctx_release(void *p) { if (enet_free) enet_free(p); else free(p); }

static int ws_reserve(rc_ctx *c, size_t n)
{
    if (n <= c->ws.n_cap) return 0;
    size_t cap = c->ws.n_cap ? c->ws.n_cap : 1024;
    while (cap < n) cap *= 2;
    uint32_t *fl = NULL, *ord = NULL, *el = NULL, *wl = NULL, *cl = NULL;
    /* claims, the decoder's reset positions and its two hand-off sums side by side */
    if (hipMalloc((void **) &cl, 5 * cap * sizeof(uint32_t)) != hipSuccess) return -1;
    if (hipMalloc((void **) &fl, cap * sizeof(uint32_t)) != hipSuccess) { hipFree(cl); return -1; }
    if (hipMalloc((void **) &ord, cap * sizeof(uint32_t)) != hipSuccess) { hipFree(cl); hipFree(fl); return -1; }
    if (hipMalloc((void **) &el, cap * sizeof(uint32_t)) != hipSuccess) {
        hipFree(cl); hipFree(fl); hipFree(ord); return -1;
    }
    if (hipMalloc((void **) &wl, cap * sizeof(uint32_t)) != hipSuccess) {
        hipFree(cl); hipFree(fl); hipFree(ord); hipFree(el); return -1;
    }
    if (c->ws.flag_list) {
        hipDeviceSynchronize();
        hipFree(c->ws.flag_list);
        hipFree(c->ws.order);
        hipFree(c->ws.enc2_list);
        hipFree(c->ws.enc2_wlist);
        hipFree(c->ws.claims);
    }
    c->ws.claims = cl;
    c->ws.dec6_resets = cl + cap;
    c->ws.dec6_icks = cl + 2 * cap;
    c->ws.dec6_hcks = cl + 3 * cap;
    c->ws.flag_list = fl;
    c->ws.order = ord;
    c->ws.enc2_list = el;
    c->ws.enc2_wlist = wl;
    c->ws.n_cap = (uint32_t) cap;
    return 0;
}

/* Per-lane model regions for the lane kernels: one per packet in flight
 * (at most one per lane of a full chip wave set; larger batches loop). */
#define MAX_LANE_SLOTS 65536u

static int lanes_reserve(rc_ctx *c, size_t n, uint32_t max_len)
{
    uint32_t region = rc_hip_lane3_region_bytes(max_len ? max_len : 4096);
    const char *ov = getenv("ENET_RC_REGION");      /* diagnostic: smaller regions (overflows take the exact path) */
    if (ov && atoi(ov) > 0 && (uint32_t) atoi(ov) < region) region = ((uint32_t) atoi(ov) + 255) & ~255u;
    /* (whole 8192-slot groups: the pieces of a split host batch differ by a
       few thousand packets between calls, and a pool that grew by each would
       be reallocated -- a device-wide wait -- on the calls after the first) */
    size_t slots = n >= 8192 ? (n + 8191) & ~(size_t) 8191 : n;
    if (slots > c->max_slots) slots = c->max_slots;
    slots = (slots + 255) & ~(size_t) 255;
    if (slots <= c->ws.lane_slots && region <= c->ws.lane_region) return 0;
    if (slots < c->ws.lane_slots) slots = c->ws.lane_slots;
    if (region < c->ws.lane_region) region = c->ws.lane_region;
    hipDeviceSynchronize();
    if (c->ws.lane_pool) hipFree(c->ws.lane_pool);
    if (c->ws.dec6_pool) hipFree(c->ws.dec6_pool);
    c->ws.lane_pool = NULL; c->ws.dec6_pool = NULL; c->ws.lane_slots = 0; c->ws.lane_region = 0;
    if (hipMalloc(&c->ws.lane_pool, slots * (size_t) region) != hipSuccess) return -1;
    /* rc_dec6.hip's bucket records: never cleared (a record's stale bytes past
       the bucket's element count are never read) */
    if (hipMalloc(&c->ws.dec6_pool, slots * (size_t) RC_DEC6_TAB_BYTES) != hipSuccess) return -1;
    /* lane regions start at epoch 0: no order-1 record is live (rc_lane3.hip) */
    if (hipMemset(c->ws.lane_pool, 0, slots * (size_t) region) != hipSuccess) return -1;
    /* hipMemset runs on the null stream, which the context's non-blocking
     * stream (and a caller's) does not wait for: finish it before any kernel */
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    c->ws.lane_slots = (uint32_t) slots;
    c->ws.lane_region = region;
    if (getenv("ENET_RC_DEBUG"))
        fprintf(stderr, "enet_rc: lane pool %p, %zu slots x %u B\n", c->ws.lane_pool, slots, region);
    return 0;
}

/* Record stream of the two-pass encoder (rc_enc2.hip): one slot per packet,
 * at most ENC2_STREAM_MAX bytes (larger batches run in whole code-pass rounds
 * of chunks; ENET_RC_ENC2_STREAM_MB=m caps it lower).  Its wide mode has a
 * stream of 16-B records for as many packets as a chunk holds (at most
 * ENC2_WIDE_MAX bytes, ENET_RC_ENC2_WIDE_MB=m caps it lower: packets past it
 * take the lane kernels; ENET_RC_ENC2_WIDE=0 turns the mode off).  Reserved
 * only for batches that take the lane path (run_device). */
/* (3 GB: a chip's worth of 4096-B packets, 65536 x 32.9 KB, in one chunk --
 * a chunk smaller than that leaves the code pass's lanes partly idle for a
 * whole packet's time) */
#define ENC2_STREAM_MAX (3ull << 30)
#define ENC2_WIDE_MAX (5ull << 30)      /* (65536 wide 4096-B packets: 4.3 GB, one chunk) */

static uint64_t env_mb_cap(const char *name, uint64_t cap)
{
    const char *mb = getenv(name);
    if (mb && atol(mb) > 0 && (uint64_t) atol(mb) << 20 < cap) cap = (uint64_t) atol(mb) << 20;
    return cap;
}

static int enc2_reserve(rc_ctx *c, size_t n, uint32_t max_len)
{
    if (!c->enc2_on || c->ws.kernel != RC_KERNEL_LANE3) return 0;
    const uint32_t ml = max_len ? max_len : 4096;
    const uint64_t slot = rc_hip_enc2_slot_bytes(ml);
    const uint64_t cap = c->enc2_stream_max;
    uint64_t want = (uint64_t) (n >= 8192 ? (n + 8191) & ~(size_t) 8191 : n) * slot;   /* (as lanes_reserve) */
    if (want > cap) want = cap > slot ? cap : slot;
    /* (a size that failed once is not retried: the stream the device could
     * give then serves, in more chunks, without a device-wide sync per call) */
    if (c->enc2_failed && want >= c->enc2_failed && c->ws.enc2_cap) want = c->ws.enc2_cap;
    if (want > c->ws.enc2_cap) {
        hipDeviceSynchronize();
        if (c->ws.enc2_stream) hipFree(c->ws.enc2_stream);
        c->ws.enc2_stream = NULL; c->ws.enc2_cap = 0;
        /* + 1 MB past the stream: the code pass's dummy store targets (rc_enc2.hip).
         * A device short of memory gets a smaller stream (the batch then runs in
         * more chunks), down to one packet's slot. */
        while (hipMalloc(&c->ws.enc2_stream, want + (1u << 20)) != hipSuccess) {
            c->ws.enc2_stream = NULL;
            (void) hipGetLastError();
            if (!c->enc2_failed || want < c->enc2_failed) c->enc2_failed = want;
            if (want <= slot) return -1;
            want = want / 2 > slot ? (want / 2) / slot * slot : slot;
        }
        c->ws.enc2_cap = want;
    }
    if (c->enc2_wide_on) {
        /* a slot per packet of a chunk, and the rounding of its RC_WSHARDS
           list regions (rc_enc2.hip wreg_cap) */
        const uint64_t wslot = rc_hip_enc2_wide_slot_bytes(ml);
        uint64_t wwant = (want / slot + RC_WSHARDS) * wslot;
        const uint64_t wcap = c->enc2_wide_max;
        if (wwant > wcap) wwant = wcap > wslot ? wcap : wslot;
        if (wwant > c->ws.enc2_wide_cap) {
            hipDeviceSynchronize();
            if (c->ws.enc2_wide) hipFree(c->ws.enc2_wide);
            c->ws.enc2_wide = NULL; c->ws.enc2_wide_cap = 0;
            /* the wide mode is optional: without its stream (an allocation that
               failed) low-entropy packets take the lane kernels */
            if (hipMalloc(&c->ws.enc2_wide, wwant) != hipSuccess) {
                c->ws.enc2_wide = NULL;
                (void) hipGetLastError();
                return 0;
            }
            c->ws.enc2_wide_cap = wwant;
        }
    }
    return 0;
}

int stage_reserve(rc_ctx *c, size_t bytes)
{
    if (bytes <= c->d_stage_cap && bytes <= c->h_stage_cap) return 0;
    size_t cap = 1u << 16;
    while (cap < bytes) cap *= 2;
    hipStreamSynchronize(c->stream);
    if (c->d_stage) hipFree(c->d_stage);
    if (c->h_stage) hipHostFree(c->h_stage);
    c->d_stage = NULL; c->h_stage = NULL; c->d_stage_cap = c->h_stage_cap = 0;
    if (hipMalloc((void **) &c->d_stage, cap) != hipSuccess) return -1;
    if (hipHostMalloc((void **) &c->h_stage, cap, 0) != hipSuccess) return -1;
    c->d_stage_cap = c->h_stage_cap = cap;
    return 0;
}

void *enet_range_coder_create(void)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return NULL;
    rc_ctx *c = (rc_ctx *) ctx_alloc(sizeof(rc_ctx));
    if (!c) return NULL;
    memset(c, 0, sizeof *c);
    c->device = dev;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) goto fail;
    /* counters[8] and the length bins in one block: one fill clears both per call */
    if (hipMalloc((void **) &c->ws.counters, RC_CTL_WORDS * sizeof(uint32_t)) != hipSuccess) goto fail;
    c->ws.bins = c->ws.counters + 8;
    c->ws.exact_slots = EXACT_SLOTS;
    if (hipMalloc(&c->ws.exact_pool, (size_t) EXACT_SLOTS * RC_EXACT_POOL_BYTES) != hipSuccess) goto fail;
    if (ws_reserve(c, 1024) != 0) goto fail;
    {
        const uint32_t words = rc_hip_crc32_table_words();
        uint32_t *t = (uint32_t *) malloc(words * sizeof(uint32_t));
        if (!t) goto fail;
        rc_hip_crc32_build_tables(t);
        hipError_t e = hipMalloc((void **) &c->crc_tables, words * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMemcpy(c->crc_tables, t, words * sizeof(uint32_t), hipMemcpyHostToDevice);
        free(t);
        if (e != hipSuccess) goto fail;
    }
    {
        const char *k = getenv("ENET_RC_KERNEL");
        c->ws.kernel = RC_KERNEL_LANE3;
        if (k && strcmp(k, "wave") == 0) c->ws.kernel = RC_KERNEL_WAVE;
        const char *a = getenv("ENET_RC_LANES");
        c->ws.lane_active = 64;
        if (a && (atoi(a) == 32 || atoi(a) == 16)) c->ws.lane_active = (uint32_t) atoi(a);
        /* ENET_RC_SMALL_BATCH=n caps the batches routed to the wave kernel
         * (0: never); unset = every batch that fits on the chip at once */
        const char *sb = getenv("ENET_RC_SMALL_BATCH");
        c->ws.small_max = sb ? (uint32_t) strtoul(sb, NULL, 10) : RC_SMALL_AUTO;
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || cus <= 0)
            cus = 256;
        c->ws.cus = (uint32_t) cus;
        const char *e2 = getenv("ENET_RC_ENC2");
        c->enc2_on = !(e2 && strcmp(e2, "0") == 0);
        c->ws.enc2_on = (uint32_t) c->enc2_on;
        const char *ew = getenv("ENET_RC_ENC2_WIDE");
        c->enc2_wide_on = !(ew && strcmp(ew, "0") == 0);
        c->enc2_stream_max = env_mb_cap("ENET_RC_ENC2_STREAM_MB", ENC2_STREAM_MAX);
        c->enc2_wide_max = env_mb_cap("ENET_RC_ENC2_WIDE_MB", ENC2_WIDE_MAX);
        /* large host batches in pieces (run_host_split): ENET_RC_HOST_SPLIT=k
           pieces, 2..SPLIT_MAX (0 or 1: off) */
        const char *hs = getenv("ENET_RC_HOST_SPLIT");
        c->split_k = hs ? atoi(hs) : SPLIT_DEFAULT;
        if (c->split_k < 1) c->split_k = 1;
        if (c->split_k > SPLIT_MAX) c->split_k = SPLIT_MAX;
        /* each piece's stream needs a hardware queue of its own (streams
           sharing one run one after the other), and the process's default
           stream holds one of the runtime's GPU_MAX_HW_QUEUES (default 4) */
        const char *hq = getenv("GPU_MAX_HW_QUEUES");
        const int queues = hq && atoi(hq) > 0 ? atoi(hq) : 4;
        if (c->split_k > queues - 1) c->split_k = queues > 2 ? queues - 1 : 1;
        /* the fast decoder: rc_dec6.hip's rc_decompress_dec6s (64 packets per
           wavefront); none with ENET_RC_DEC=0 (ENET_RC_DEC4=0, the older name,
           too) or with 32 / 16 packets per wavefront */
        const char *d4 = getenv("ENET_RC_DEC4");
        const char *dk = getenv("ENET_RC_DEC");
        c->ws.fast_dec = c->ws.lane_active == 64;
        if ((dk && strcmp(dk, "0") == 0) || (d4 && strcmp(d4, "0") == 0)) c->ws.fast_dec = 0;
        const char *dd = getenv("ENET_RC_DEC6_DEBUG");
        c->ws.dec6_debug = dd ? (uint32_t) atoi(dd) : 0u;
        const char *es = getenv("ENET_RC_ENC2_SLOW");
        c->ws.enc2_slow = (es && strcmp(es, "1") == 0) ? 1u : 0u;
        const char *sl = getenv("ENET_RC_SLOTS");
        c->max_slots = MAX_LANE_SLOTS;
        if (sl && atol(sl) >= 256 && atol(sl) <= (1l << 22)) c->max_slots = (uint32_t) atol(sl);
    }
    if (stage_reserve(c, 1u << 16) != 0) goto fail;
    return c;
fail:
    enet_range_coder_destroy(c);
    return NULL;
}

/* The settings enet_range_coder_create reads from the environment, copied
 * from a context to another on the same device (run_host_split's second
 * half runs with its parent's configuration, whatever the environment says
 * by then). */
void ctx_copy_config(rc_ctx *dst, const rc_ctx *src)
{
    dst->ws.kernel = src->ws.kernel;
    dst->ws.lane_active = src->ws.lane_active;
    dst->ws.small_max = src->ws.small_max;
    dst->ws.cus = src->ws.cus;
    dst->ws.fast_dec = src->ws.fast_dec;
    dst->ws.dec6_debug = src->ws.dec6_debug;
    dst->ws.enc2_slow = src->ws.enc2_slow;
    dst->enc2_on = src->enc2_on;
    dst->ws.enc2_on = src->ws.enc2_on;
    dst->enc2_wide_on = src->enc2_wide_on;
    dst->enc2_stream_max = src->enc2_stream_max;
    dst->enc2_wide_max = src->enc2_wide_max;
    dst->max_slots = src->max_slots;
    dst->split_k = 1;
}

void enet_range_coder_destroy(void *context)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->ws.flag_list) hipFree(c->ws.flag_list);
    if (c->ws.counters) hipFree(c->ws.counters);
    if (c->ws.order) hipFree(c->ws.order);
    if (c->ws.enc2_list) hipFree(c->ws.enc2_list);
    if (c->ws.claims) hipFree(c->ws.claims);
    if (c->ws.dec6_pool) hipFree(c->ws.dec6_pool);
    if (c->ws.enc2_stream) hipFree(c->ws.enc2_stream);
    if (c->ws.enc2_wlist) hipFree(c->ws.enc2_wlist);
    if (c->ws.enc2_wide) hipFree(c->ws.enc2_wide);
    if (c->ws.exact_pool) hipFree(c->ws.exact_pool);
    if (c->ws.lane_pool) hipFree(c->ws.lane_pool);
    if (c->crc_tables) hipFree(c->crc_tables);
    if (c->dg_arrays) hipFree(c->dg_arrays);
    if (c->dg_scratch) hipFree(c->dg_scratch);
    if (c->d_pack) hipFree(c->d_pack);
    if (c->d_bsum) hipFree(c->d_bsum);
    if (c->d_stage) hipFree(c->d_stage);
    if (c->h_stage) hipHostFree(c->h_stage);
    if (c->stream) hipStreamDestroy(c->stream);
    for (int i = 0; i < SPLIT_MAX - 1; ++i)
        if (c->twin[i]) enet_range_coder_destroy(c->twin[i]);
    ctx_release(c);
}

/* (as rc_fail, for the device-pointer path) */
static int rc_fail_dev(int err, int line)
{
    if (err && getenv("ENET_RC_DEBUG"))
        fprintf(stderr, "enet_rc: batch failed at rc_host.c:%d: %d (%s)\n", line, err, hipGetErrorString((hipError_t) err));
    return err;
}

int run_device(rc_ctx *c, int decompress, const uint8_t *in, const uint64_t *in_off,
                      const uint32_t *in_len, size_t n, uint32_t max_len, uint32_t max_out, uint8_t *out,
                      const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len,
                      void *stream)
{
    if (!c) return (int) hipErrorInvalidValue;
    c->last_split = 0;
    if (n == 0) return 0;
    if (n > 0xFFFFFFFFu) return (int) hipErrorInvalidValue;
    if (hipSetDevice(c->device) != hipSuccess) return (int) hipErrorInvalidDevice;
    if (ws_reserve(c, n) != 0) return rc_fail_dev((int) hipErrorOutOfMemory, __LINE__);
    rc_batch_dev b;
    b.in = in; b.in_off = in_off; b.in_len = in_len;
    b.out = out; b.out_off = out_off; b.out_cap = out_cap; b.out_len = out_len;
    b.n = (uint32_t) n;
    b.max_len = max_len;
    b.max_out = max_out;
    /* the lane pool and the encoder's record stream only for batches that run
     * on the lane path (small batches run on the wave kernel without them) */
    if (rc_hip_uses_lanes(decompress, &b, &c->ws)) {
        if (lanes_reserve(c, n, max_len) != 0) return rc_fail_dev((int) hipErrorOutOfMemory, __LINE__);
        if (!decompress && enc2_reserve(c, n, max_len) != 0) return rc_fail_dev((int) hipErrorOutOfMemory, __LINE__);
    }
    /* stream is a hipStream_t; NULL is HIP's default (null) stream */
    return decompress ? rc_hip_decompress(&b, &c->ws, stream) : rc_hip_compress(&b, &c->ws, stream);
}

int enet_rc_compress_batch_device(void *context, const uint8_t *in, const uint64_t *in_off,
                                  const uint32_t *in_len, size_t n, uint32_t max_len,
                                  uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                                  uint32_t *out_len, void *stream)
{
    return run_device((rc_ctx *) context, 0, in, in_off, in_len, n, max_len, 0, out, out_off,
                      out_cap, out_len, stream);
}

int enet_rc_decompress_batch_device(void *context, const uint8_t *in, const uint64_t *in_off,
                                    const uint32_t *in_len, size_t n, uint32_t max_len,
                                    uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                                    uint32_t *out_len, void *stream)
{
    return run_device((rc_ctx *) context, 1, in, in_off, in_len, n, max_len, 0, out, out_off,
                      out_cap, out_len, stream);
}

int enet_rc_decompress_batch_device_bounded(void *context, const uint8_t *in, const uint64_t *in_off,
                                            const uint32_t *in_len, size_t n, uint32_t max_len,
                                            uint8_t *out, const uint64_t *out_off, const uint32_t *out_cap,
                                            uint32_t *out_len, uint32_t max_out, void *stream)
{
    return run_device((rc_ctx *) context, 1, in, in_off, in_len, n, max_len, max_out, out, out_off,
                      out_cap, out_len, stream);
}

int pack_reserve(rc_ctx *c, size_t bytes, size_t blocks)
{
    if (bytes > c->d_pack_cap) {
        hipStreamSynchronize(c->stream);
        if (c->d_pack) hipFree(c->d_pack);
        c->d_pack = NULL; c->d_pack_cap = 0;
        if (hipMalloc((void **) &c->d_pack, bytes) != hipSuccess) return -1;
        c->d_pack_cap = bytes;
    }
    if (blocks + 1 > c->d_bsum_cap) {
        hipStreamSynchronize(c->stream);
        if (c->d_bsum) hipFree(c->d_bsum);
        c->d_bsum = NULL; c->d_bsum_cap = 0;
        if (hipMalloc((void **) &c->d_bsum, (blocks + 1) * 8) != hipSuccess) return -1;
        c->d_bsum_cap = blocks + 1;
    }
    return 0;
}

int rc_fail(int err, const char *file, int line)
{
    if (err && rc_host_cfg()->debug)
        fprintf(stderr, "enet_rc: host batch failed at %s:%d: %d (%s)\n", file, line, err,
                hipGetErrorString((hipError_t) err));
    return err;
}

/* --------------------------------------------------- datagram framing (§8f) */

#define DG_MTU 4096u                /* ENET_PROTOCOL_MAXIMUM_MTU (protocol.h:13) */

static int dgram_reserve(rc_ctx *c, size_t n, int scratch)
{
    if (n > c->dg_cap) {
        size_t cap = c->dg_cap ? c->dg_cap : 1024;
        while (cap < n) cap *= 2;
        hipDeviceSynchronize();             /* (the device calls run on the caller's stream) */
        if (c->dg_arrays) hipFree(c->dg_arrays);
        c->dg_arrays = NULL; c->dg_cap = 0;
        if (hipMalloc((void **) &c->dg_arrays, cap * (3 * 8 + 6 * 4)) != hipSuccess) return -1;
        c->dg_cap = cap;
    }
    if (scratch && n * DG_MTU > c->dg_scratch_cap) {
        hipDeviceSynchronize();
        if (c->dg_scratch) hipFree(c->dg_scratch);
        c->dg_scratch = NULL; c->dg_scratch_cap = 0;
        if (hipMalloc((void **) &c->dg_scratch, n * DG_MTU) != hipSuccess) return -1;
        c->dg_scratch_cap = n * DG_MTU;
    }
    return 0;
}

/* protocol.c:1686-1718 (send) or :1022-1091 (receive) for a batch of whole
 * datagrams: frame, code the command ranges with the lane kernels, checksum. */
static int run_dgram(rc_ctx *c, int decode, const uint8_t *in, const uint64_t *in_off,
                     const uint32_t *in_len, size_t n, int checksum, const uint32_t *seed,
                     uint8_t *out, const uint64_t *out_off, uint32_t *out_len, void *stream)
{
    if (!c || n > 0xFFFFFFFFu || (checksum && !seed)) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return (int) hipErrorInvalidDevice;
    if (dgram_reserve(c, n, checksum && !decode) != 0) return (int) hipErrorOutOfMemory;
    uint8_t *a = c->dg_arrays;
    const size_t cap = c->dg_cap;
    rc_dgram_dev g;
    g.in = in; g.in_off = in_off; g.in_len = in_len;
    g.out = out; g.out_off = out_off; g.out_len = out_len;
    g.seed = seed;
    g.p_off = (uint64_t *) a;
    g.q_off = (uint64_t *) (a + cap * 8);
    g.s_off = (uint64_t *) (a + cap * 16);
    g.p_len = (uint32_t *) (a + cap * 24);
    g.q_cap = (uint32_t *) (a + cap * 28);
    g.c_len = (uint32_t *) (a + cap * 32);
    g.s_len = (uint32_t *) (a + cap * 36);
    g.crc = (uint32_t *) (a + cap * 40);
    g.want = (uint32_t *) (a + cap * 44);
    g.scratch = c->dg_scratch;
    g.n = (uint32_t) n;
    g.checksum = checksum ? 1u : 0u;
    int rc = rc_hip_dgram_launch(decode ? RC_DGRAM_DEC_PREP : RC_DGRAM_ENC_PREP, &g, stream);
    if (rc) return rc;
    rc = run_device(c, decode, in, g.p_off, g.p_len, n, DG_MTU, 0, out, g.q_off, g.q_cap, g.c_len, stream);
    if (rc) return rc;
    rc = rc_hip_dgram_launch(decode ? RC_DGRAM_DEC_STAGE : RC_DGRAM_ENC_STAGE, &g, stream);
    if (rc) return rc;
    if (checksum) {
        rc = decode ? rc_hip_crc32(out, out_off, g.s_len, (uint32_t) n, g.crc, c->crc_tables, stream)
                    : rc_hip_crc32(g.scratch, g.s_off, g.s_len, (uint32_t) n, g.crc, c->crc_tables, stream);
        if (rc) return rc;
        rc = rc_hip_dgram_launch(decode ? RC_DGRAM_DEC_FINISH : RC_DGRAM_ENC_FINISH, &g, stream);
    }
    return rc;
}

int enet_rc_datagram_encode_batch_device(void *context, const uint8_t *in, const uint64_t *in_off,
                                         const uint32_t *in_len, size_t n, int checksum,
                                         const uint32_t *seed, uint8_t *out, const uint64_t *out_off,
                                         uint32_t *out_len, void *stream)
{
    return run_dgram((rc_ctx *) context, 0, in, in_off, in_len, n, checksum, seed, out, out_off,
                     out_len, stream);
}

int enet_rc_datagram_decode_batch_device(void *context, const uint8_t *in, const uint64_t *in_off,
                                         const uint32_t *in_len, size_t n, int checksum,
                                         const uint32_t *seed, uint8_t *out, const uint64_t *out_off,
                                         uint32_t *out_len, void *stream)
{
    return run_dgram((rc_ctx *) context, 1, in, in_off, in_len, n, checksum, seed, out, out_off,
                     out_len, stream);
}

/* Host-pointer variants: one pinned staging area, H2D, the device path, D2H
 * of the lengths and of each slot's used bytes only. */
static int run_dgram_host(rc_ctx *c, int decode, const uint8_t *in, const uint64_t *in_off,
                          const uint32_t *in_len, size_t n, int checksum, const uint32_t *seed,
                          uint8_t *out, const uint64_t *out_off, uint32_t *out_len)
{
    if (!c || n > 0xFFFFFFFFu || (checksum && !seed)) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    uint64_t in_bytes = 0, out_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        uint64_t e = in_off[i] + in_len[i];
        if (e > in_bytes) in_bytes = e;
        uint64_t f = out_off[i] + (decode ? DG_MTU : in_len[i]);
        if (f > out_bytes) out_bytes = f;
    }
    size_t a_ioff = (in_bytes + 15) & ~(size_t) 15;
    size_t a_ilen = a_ioff + n * 8;
    size_t a_seed = (a_ilen + n * 4 + 15) & ~(size_t) 15;
    size_t a_ooff = (a_seed + n * 4 + 15) & ~(size_t) 15;
    size_t a_olen = (a_ooff + n * 8 + 15) & ~(size_t) 15;
    size_t a_out = (a_olen + n * 4 + 15) & ~(size_t) 15;
    size_t total = a_out + out_bytes + 16;
    size_t a_soff = (total + 15) & ~(size_t) 15;        /* source offsets of a device-side gather */
    if (hipSetDevice(c->device) != hipSuccess) return (int) hipErrorInvalidDevice;
    if (stage_reserve(c, a_soff + n * 8) != 0) return (int) hipErrorOutOfMemory;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    memcpy(h, in, in_bytes);
    memcpy(h + a_ioff, in_off, n * 8);
    memcpy(h + a_ilen, in_len, n * 4);
    if (checksum) memcpy(h + a_seed, seed, n * 4);
    memcpy(h + a_ooff, out_off, n * 8);
    hipError_t err = hipMemcpyAsync(d, h, a_olen, hipMemcpyHostToDevice, c->stream);
    if (err != hipSuccess) return (int) err;
    int rc = run_dgram(c, decode, d, (const uint64_t *) (d + a_ioff), (const uint32_t *) (d + a_ilen), n,
                       checksum, (const uint32_t *) (d + a_seed), d + a_out, (const uint64_t *) (d + a_ooff),
                       (uint32_t *) (d + a_olen), (void *) c->stream);
    if (rc) return rc;
    err = hipMemcpyAsync(h + a_olen, d + a_olen, total - 16 - a_olen, hipMemcpyDeviceToHost, c->stream);
    if (err != hipSuccess) return (int) err;
    err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) return (int) err;
    memcpy(out_len, h + a_olen, n * 4);
    for (size_t i = 0; i < n; ++i)
        if (out_len[i]) memcpy(out + out_off[i], h + a_out + out_off[i], out_len[i]);
    return 0;
}

int enet_rc_datagram_encode_batch_host(void *context, const uint8_t *in, const uint64_t *in_off,
                                       const uint32_t *in_len, size_t n, int checksum, const uint32_t *seed,
                                       uint8_t *out, const uint64_t *out_off, uint32_t *out_len)
{
    return run_dgram_host((rc_ctx *) context, 0, in, in_off, in_len, n, checksum, seed, out, out_off, out_len);
}

int enet_rc_datagram_decode_batch_host(void *context, const uint8_t *in, const uint64_t *in_off,
                                       const uint32_t *in_len, size_t n, int checksum, const uint32_t *seed,
                                       uint8_t *out, const uint64_t *out_off, uint32_t *out_len)
{
    return run_dgram_host((rc_ctx *) context, 1, in, in_off, in_len, n, checksum, seed, out, out_off, out_len);
}

/* ------------------------------------------------------------------ CRC-32 */

int enet_rc_crc32_batch_device(void *context, const uint8_t *in, const uint64_t *in_off,
                               const uint32_t *in_len, size_t n, uint32_t *crc_out, void *stream)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c || n > 0xFFFFFFFFu) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    if (hipSetDevice(c->device) != hipSuccess) return (int) hipErrorInvalidDevice;
    return rc_hip_crc32(in, in_off, in_len, (uint32_t) n, crc_out, c->crc_tables, stream);
}

int enet_rc_crc32_batch_host(void *context, const uint8_t *in, const uint64_t *in_off,
                             const uint32_t *in_len, size_t n, uint32_t *crc_out)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c || n > 0xFFFFFFFFu) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    uint64_t in_bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        uint64_t e = in_off[i] + in_len[i];
        if (e > in_bytes) in_bytes = e;
    }
    size_t a_ioff = (in_bytes + 15) & ~(size_t) 15;
    size_t a_ilen = a_ioff + n * 8;
    size_t a_crc = (a_ilen + n * 4 + 15) & ~(size_t) 15;
    size_t total = a_crc + n * 4;
    if (hipSetDevice(c->device) != hipSuccess) return (int) hipErrorInvalidDevice;
    if (stage_reserve(c, total) != 0) return (int) hipErrorOutOfMemory;
    uint8_t *h = c->h_stage, *d = c->d_stage;
    memcpy(h, in, in_bytes);
    memcpy(h + a_ioff, in_off, n * 8);
    memcpy(h + a_ilen, in_len, n * 4);
    hipError_t err = hipMemcpyAsync(d, h, a_crc, hipMemcpyHostToDevice, c->stream);
    if (err != hipSuccess) return (int) err;
    int rc = rc_hip_crc32(d, (const uint64_t *) (d + a_ioff), (const uint32_t *) (d + a_ilen), (uint32_t) n,
                          (uint32_t *) (d + a_crc), c->crc_tables, (void *) c->stream);
    if (rc != 0) return rc;
    err = hipMemcpyAsync(h + a_crc, d + a_crc, n * 4, hipMemcpyDeviceToHost, c->stream);
    if (err != hipSuccess) return (int) err;
    err = hipStreamSynchronize(c->stream);
    if (err != hipSuccess) return (int) err;
    memcpy(crc_out, h + a_crc, n * 4);
    return 0;
}

/* ENetChecksumCallback (enet.h:338) with no context argument: a process-wide
 * context, created on first use.  Gather lists are checksummed as one stream,
 * like enet_crc32's loop over buffers (packet.c:148-160). */
static pthread_once_t crc_once = PTHREAD_ONCE_INIT;
static void *crc_ctx;
static pthread_mutex_t crc_lock = PTHREAD_MUTEX_INITIALIZER;
static void crc_ctx_init(void) { crc_ctx = enet_range_coder_create(); }

enet_uint32 enet_rc_crc32(const ENetBuffer *buffers, size_t bufferCount)
{
    pthread_once(&crc_once, crc_ctx_init);
    size_t total = 0;
    for (size_t i = 0; i < bufferCount; ++i) total += buffers[i].dataLength;
    if (!crc_ctx || total > 0xFFFFFFFFu) abort();          /* no silent CPU fallback */
    uint8_t *flat = (uint8_t *) malloc(total ? total : 1);
    if (!flat) abort();
    size_t pos = 0;
    for (size_t i = 0; i < bufferCount; ++i) {
        if (buffers[i].dataLength) memcpy(flat + pos, buffers[i].data, buffers[i].dataLength);
        pos += buffers[i].dataLength;
    }
    uint64_t off = 0;
    uint32_t len = (uint32_t) total, crc = 0;
    pthread_mutex_lock(&crc_lock);
    int rc = enet_rc_crc32_batch_host(crc_ctx, flat, &off, &len, 1, &crc);
    pthread_mutex_unlock(&crc_lock);
    free(flat);
    if (rc != 0) abort();
    return crc;
}

/* --------------------------------------------------------- per-datagram ABI */

size_t enet_range_coder_compress(void *context, const ENetBuffer *inBuffers, size_t inBufferCount,
                                 size_t inLimit, enet_uint8 *outData, size_t outLimit)
{
    rc_ctx *c = (rc_ctx *) context;
    if (c == NULL || inBufferCount <= 0 || inLimit <= 0) return 0;      /* compress.c:257-258 */
    /* the gather list is flattened into the staging the way compress.c:275-284
     * walks it (rc_gather_len / rc_gather_copy, rc_hostcopy.c) */
    const size_t total = rc_gather_len(inBuffers, inBufferCount);
    if (total > 0xFFFFFFFFu || outLimit > 0xFFFFFFFFu) return 0;
    if (total == 0) return 0;   /* only an empty first buffer: compress.c flushes nothing */
    const size_t first[2] = {0, inBufferCount};
    uint64_t ooff = 0;
    uint32_t ocap = (uint32_t) outLimit, olen = 0;
    const int rc = enet_rc_compress_gather_batch_host(c, inBuffers, first, 1, outData, &ooff, &ocap, &olen);
    return rc == 0 ? (size_t) olen : 0;
}

size_t enet_range_coder_decompress(void *context, const enet_uint8 *inData, size_t inLimit,
                                   enet_uint8 *outData, size_t outLimit)
{
    rc_ctx *c = (rc_ctx *) context;
    if (c == NULL || inLimit <= 0) return 0;                             /* compress.c:513-514 */
    if (inLimit > 0xFFFFFFFFu) return 0;
    uint64_t ioff = 0, ooff = 0;
    uint32_t ilen = (uint32_t) inLimit, ocap = (uint32_t) (outLimit > 0xFFFFFFFFu ? 0xFFFFFFFFu : outLimit);
    uint32_t olen = 0;
    int rc = enet_rc_decompress_batch_host(c, inData, &ioff, &ilen, 1, outData, &ooff, &ocap, &olen);
    return rc == 0 ? (size_t) olen : 0;
}

int enet_host_compress_with_range_coder(ENetHost *host)
{
    ENetCompressor compressor;
    if (!enet_host_compress) return -1;
    memset(&compressor, 0, sizeof compressor);
    compressor.context = enet_range_coder_create();
    if (compressor.context == NULL) return -1;
    compressor.compress = enet_range_coder_compress;
    compressor.decompress = enet_range_coder_decompress;
    compressor.destroy = enet_range_coder_destroy;
    enet_host_compress(host, &compressor);
    return 0;
}

uint32_t enet_rc_last_lane_count(void *context)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c) return 0;
    uint32_t v = 0, w = 0;
    hipDeviceSynchronize();
    if (hipMemcpy(&v, c->ws.counters + 3, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int i = 0; i + 1 < c->last_split; ++i) {
        if (!c->twin[i] ||
            hipMemcpy(&w, ((rc_ctx *) c->twin[i])->ws.counters + 3, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
        v += w;
    }
    return v;
}

uint32_t enet_rc_last_exact_count(void *context)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c) return 0;
    uint32_t v = 0, w = 0;
    hipDeviceSynchronize();
    if (hipMemcpy(&v, c->ws.counters, 4, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    for (int i = 0; i + 1 < c->last_split; ++i) {
        if (!c->twin[i] || hipMemcpy(&w, ((rc_ctx *) c->twin[i])->ws.counters, 4, hipMemcpyDeviceToHost) != hipSuccess)
            return 0;
        v += w;
    }
    return v;
}

/* The context's kernel configuration as flag bits (the settings
 * enet_range_coder_create read from the environment); bit 31: the context
 * that runs the second half of its split host batches (run_host_split) has a
 * different one. */
static uint32_t config_flags(const rc_ctx *c)
{
    return (c->ws.kernel == RC_KERNEL_WAVE ? 1u : 0u) | (c->enc2_on ? 2u : 0u) | (c->enc2_wide_on ? 4u : 0u) |
           (c->ws.fast_dec ? 8u : 0u) | (c->ws.enc2_slow ? 16u : 0u) | ((c->ws.lane_active & 0x7Fu) << 8);
}

uint32_t enet_rc_config_flags(void *context)
{
    const rc_ctx *c = (const rc_ctx *) context;
    if (!c) return 0;
    const uint32_t f = config_flags(c);
    int differ = 0;
    for (int i = 0; i < SPLIT_MAX - 1; ++i) {
        const rc_ctx *t = (const rc_ctx *) c->twin[i];
        differ |= t && (config_flags(t) != f || t->enc2_stream_max != c->enc2_stream_max ||
                        t->enc2_wide_max != c->enc2_wide_max || t->max_slots != c->max_slots ||
                        t->ws.small_max != c->ws.small_max || t->ws.dec6_debug != c->ws.dec6_debug);
    }
    return f | (differ ? 0x80000000u : 0u);
}

uint32_t enet_rc_last_split(void *context) { return context ? (uint32_t) ((rc_ctx *) context)->last_split : 0u; }

uint32_t enet_rc_debug_counter(void *context, uint32_t i)
{
    rc_ctx *c = (rc_ctx *) context;
    uint32_t v = 0;
    if (!c || i >= 8 || !c->ws.counters || hipSetDevice(c->device) != hipSuccess) return 0;
    if (hipStreamSynchronize(c->stream) != hipSuccess ||
        hipMemcpy(&v, c->ws.counters + i, 4, hipMemcpyDeviceToHost) != hipSuccess) {
        (void) hipGetLastError();
        return 0;
    }
    return v;
}

uint32_t enet_rc_last_host_paths(void *context)
{
    const rc_ctx *c = (const rc_ctx *) context;
    if (!c) return 0;
    /* a split batch: its last piece's */
    for (int i = c->last_split - 2; i >= 0; --i)
        if (c->twin[i]) return ((const rc_ctx *) c->twin[i])->last_paths;
    return c->last_paths;
}

/* ------------------------------------------------------ for rc_multi.c */

int rc_ctx_device(void *context) { return context ? ((rc_ctx *) context)->device : -1; }
void *rc_ctx_stream(void *context) { return context ? (void *) ((rc_ctx *) context)->stream : NULL; }

int rc_ctx_run_device(void *context, int decompress, const uint8_t *in, const uint64_t *in_off,
                      const uint32_t *in_len, size_t n, uint32_t max_len, uint8_t *out,
                      const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, void *stream)
{
    return run_device((rc_ctx *) context, decompress, in, in_off, in_len, n, max_len, 0, out, out_off, out_cap,
                      out_len, stream);
}


/* The context's block-sum workspace of rc_pack.hip for n packets (device
 * pointer, ceil(n / 1024) + 1 words; the last holds the packed total). */
uint64_t *rc_ctx_bsum(void *context, size_t n)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c || hipSetDevice(c->device) != hipSuccess) return NULL;
    const size_t blocks = (n + 1023) / 1024;
    if (blocks + 1 > c->d_bsum_cap) {
        hipDeviceSynchronize();
        if (c->d_bsum) hipFree(c->d_bsum);
        c->d_bsum = NULL; c->d_bsum_cap = 0;
        if (hipMalloc((void **) &c->d_bsum, (blocks + 1) * 8) != hipSuccess) return NULL;
        c->d_bsum_cap = blocks + 1;
    }
    return c->d_bsum;
}

/* Packs out_len[i] bytes of each packet back to back (rc_pack.hip). */
int enet_rc_pack_batch_device(void *context, const uint8_t *out, const uint64_t *out_off, const uint32_t *out_len,
                              size_t n, uint8_t *packed, void *stream)
{
    rc_ctx *c = (rc_ctx *) context;
    if (!c || n > 0xFFFFFFFFu) return (int) hipErrorInvalidValue;
    if (n == 0) return 0;
    uint64_t *bsum = rc_ctx_bsum(c, n);
    if (!bsum) return (int) hipErrorOutOfMemory;
    return rc_hip_pack(out, out_off, out_len, (uint32_t) n, bsum, packed, stream);
}

const char *enet_rc_version(void) { return "enet_rc_amd 0.3 (gfx950)"; }
