/*
 * rc_host_internal.h -- what the host shim's files share:
 *   - the coder context and its reserves (rc_host.c), for the host-memory
 *     batch path (rc_hostmem.c); seen only by files that include the HIP
 *     runtime API before this header;
 *   - the host-path switches and the copy threads (rc_hostcopy.c, plain C);
 *   - what rc_multi.c uses of a coder context.
 * Plain C, plain pointers.
 */
#ifndef ENET_RC_HOST_INTERNAL_H
#define ENET_RC_HOST_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "enet_rc_amd.h"

/* ---- rc_hostcopy.c: host-path switches, read once per process on first use */
struct host_cfg {
    int no_pin;                     /* ENET_RC_NO_HOST_PIN: caller memory never DMA'd directly */
    int gpu_copy;                   /* ENET_RC_GPU_COPY=0: gapped inputs and outputs through pinned staging
                                       on the host, not the GPU's gather / slot-copy kernels */
    int h2d_dma;                    /* ENET_RC_H2D_DMA=0: plain input copies, not 2D ones */
    int contig_dma;                 /* ENET_RC_CONTIG_DMA=0: back-to-back slots take the slot copy too */
    int copy_threads;               /* ENET_RC_COPY_THREADS, 1..16 (default 8) */
    int profile;                    /* ENET_RC_HOST_PROFILE: phase times of a host batch on stderr */
    int debug;                      /* ENET_RC_DEBUG: a failed host batch's line on stderr */
    uint32_t piece_copy_wgs;        /* ENET_RC_PIECE_COPY_WGS: workgroups of a piece's slot copy
                                       (default 64; 0: 8 per CU) */
};
const struct host_cfg *rc_host_cfg(void);

/* ---- rc_hostcopy.c: copies on the copy threads */
#define RC_COPY_MIN_BYTES (4u << 20)    /* smaller copies run on the caller's thread */
size_t rc_gather_len(const ENetBuffer *b, size_t k);
void rc_gather_copy(uint8_t *dst, const ENetBuffer *b, size_t k);
void rc_par_memcpy(uint8_t *dst, const uint8_t *src, size_t bytes);
/* packets [lo, hi): out + out_off[i] <- packed + poff[i], len[i] bytes */
void rc_par_scatter(uint8_t *out, const uint64_t *out_off, const uint8_t *packed, const uint64_t *poff,
                    const uint32_t *len, size_t lo, size_t hi, uint64_t bytes);
/* packets [lo, hi) of gather lists flattened into dst + poff[i] */
void rc_par_gather(uint8_t *dst, const uint64_t *poff, const ENetBuffer *gbuf, const size_t *gfirst,
                   size_t lo, size_t hi, uint64_t bytes);

/* ---- rc_host.c: for rc_multi.c */
int rc_ctx_device(void *context);
void *rc_ctx_stream(void *context);
/* enet_rc_{compress,decompress}_batch_device / _host of one context */
int rc_ctx_run_device(void *context, int decompress, const uint8_t *in, const uint64_t *in_off,
                      const uint32_t *in_len, size_t n, uint32_t max_len, uint8_t *out,
                      const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, void *stream);
int rc_ctx_run_host(void *context, int decompress, const uint8_t *in, const uint64_t *in_off,
                    const uint32_t *in_len, size_t n, uint8_t *out, const uint64_t *out_off,
                    const uint32_t *out_cap, uint32_t *out_len);

/* rc_pack.hip's block-sum workspace of the context, for n packets (NULL: out of memory) */
uint64_t *rc_ctx_bsum(void *context, size_t n);

#ifdef HIP_INCLUDE_HIP_HIP_RUNTIME_API_H
#include <pthread.h>
#include "rc_abi_internal.h"

/* ---- rc_host.c: the coder context */
#define SPLIT_MAX 4                 /* pieces of a large host batch (run_host_split) */

/* A piece records ev on its stream once its input DMA is enqueued (ready 1;
 * -1: it ended before that), the next piece's stream waits for it before its
 * own. */
struct h2d_sync {
    pthread_mutex_t m;
    pthread_cond_t cv;
    int ready;
    hipEvent_t ev;
};

typedef struct {
    int device;
    hipStream_t stream;
    rc_workspace_dev ws;            /* flag list sized n_cap */
    /* device staging for host-pointer calls */
    uint8_t *d_stage;
    size_t d_stage_cap;
    uint8_t *h_stage;               /* pinned */
    size_t h_stage_cap;
    uint32_t last_exact;
    uint32_t max_slots;             /* lanes with a model region (ENET_RC_SLOTS) */
    int enc2_on;                    /* compress batches on the two-pass encoder (ENET_RC_ENC2=0: off) */
    int enc2_wide_on;               /* ... and its wide mode (ENET_RC_ENC2_WIDE=0: off) */
    uint64_t enc2_stream_max;       /* record-stream caps, read when the context is created */
    uint64_t enc2_wide_max;
    uint64_t enc2_failed;     /* the smallest record-stream size an allocation failed for (0: none) */
    uint32_t *crc_tables;           /* device: slice-by-16 + shift tables (rc_crc32.hip) */
    /* datagram framing workspace (rc_dgram.hip): per-datagram arrays + checksum scratch */
    uint8_t *dg_arrays;
    size_t dg_cap;
    uint8_t *dg_scratch;
    size_t dg_scratch_cap;
    /* host-pointer calls: outputs packed back to back before D2H (rc_pack.hip) */
    uint8_t *d_pack;
    size_t d_pack_cap;
    uint64_t *d_bsum;
    size_t d_bsum_cap;
    /* host batches in pieces (run_host_split): the further contexts on the
       device, and the hand-off of each piece's input DMA to the next piece */
    void *twin[SPLIT_MAX - 1];
    struct h2d_sync *sync_sig, *sync_wait;
    int last_split;                 /* pieces of the last host batch (0: one piece) */
    uint32_t last_paths;            /* enet_rc_last_host_paths */
    int split_k;                    /* pieces of a large host batch (ENET_RC_HOST_SPLIT) */
} rc_ctx;

int stage_reserve(rc_ctx *c, size_t bytes);
int pack_reserve(rc_ctx *c, size_t bytes, size_t blocks);
int run_device(rc_ctx *c, int decompress, const uint8_t *in, const uint64_t *in_off,
               const uint32_t *in_len, size_t n, uint32_t max_len, uint32_t max_out, uint8_t *out,
               const uint64_t *out_off, const uint32_t *out_cap, uint32_t *out_len, void *stream);
/* A batch's failure, with the place that saw it, on stderr when ENET_RC_DEBUG
 * is set (a failed call returns the HIP error either way) */
int rc_fail(int err, const char *file, int line);
/* The settings enet_range_coder_create read from the environment, copied to
 * another context on the same device */
void ctx_copy_config(rc_ctx *dst, const rc_ctx *src);
#endif

#endif
