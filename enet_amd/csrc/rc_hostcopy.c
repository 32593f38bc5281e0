/*
 * rc_hostcopy.c -- the host-memory path's CPU side: its switches, and the
 * host-side copies on several threads (the staging memcpy in and the scatter
 * of the packed results out are the largest host costs of a host batch).
 * Plain C11 and pthreads, no HIP: it builds and runs without a GPU
 * (tests/proto/hostcopy_main.c).
 */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <stdlib.h>
#include <string.h>

#include "rc_host_internal.h"

#define COPY_THREADS_MAX 16

static struct host_cfg cfg;
static pthread_once_t cfg_once = PTHREAD_ONCE_INIT;

static int env_on(const char *name, int dflt)
{
    const char *e = getenv(name);
    return e ? atoi(e) != 0 : dflt;
}

static void cfg_read(void)
{
    cfg.no_pin = getenv("ENET_RC_NO_HOST_PIN") != NULL;
    cfg.gpu_copy = env_on("ENET_RC_GPU_COPY", 1);
    cfg.h2d_dma = env_on("ENET_RC_H2D_DMA", 1);
    cfg.contig_dma = env_on("ENET_RC_CONTIG_DMA", 1);
    const char *t = getenv("ENET_RC_COPY_THREADS");
    const int k = t ? atoi(t) : 8;
    cfg.copy_threads = k < 1 ? 1 : (k > COPY_THREADS_MAX ? COPY_THREADS_MAX : k);
    cfg.profile = getenv("ENET_RC_HOST_PROFILE") != NULL;
    cfg.debug = getenv("ENET_RC_DEBUG") != NULL;
    const char *w = getenv("ENET_RC_PIECE_COPY_WGS");
    const long wgs = w ? atol(w) : 64;
    cfg.piece_copy_wgs = wgs < 0 ? 0u : (uint32_t) wgs;
}

const struct host_cfg *rc_host_cfg(void)
{
    pthread_once(&cfg_once, cfg_read);
    return &cfg;
}

typedef struct {
    int kind;                       /* 0: memcpy range, 1: scatter packets, 2: flatten gather lists */
    uint8_t *dst;
    const uint8_t *src;
    size_t bytes;
    const uint64_t *out_off, *poff;
    const uint32_t *len;
    size_t lo, hi;
    const ENetBuffer *gbuf;         /* kind 2: packet i = gbuf[gfirst[i] .. gfirst[i + 1]) */
    const size_t *gfirst;
} copy_job;

/* packet i's gather list flattened the way compress.c:260-285 walks it: the
 * first buffer as it is (empty: nothing), every later buffer at least its
 * data[0] (an empty one still yields that byte, the phantom byte) */
size_t rc_gather_len(const ENetBuffer *b, size_t k)
{
    if (k == 0) return 0;
    size_t total = b[0].dataLength;
    for (size_t j = 1; j < k; ++j) total += b[j].dataLength ? b[j].dataLength : 1;
    return total;
}

void rc_gather_copy(uint8_t *dst, const ENetBuffer *b, size_t k)
{
    if (k == 0) return;
    size_t pos = b[0].dataLength;
    if (pos) memcpy(dst, b[0].data, pos);
    for (size_t j = 1; j < k; ++j) {
        const size_t l = b[j].dataLength;
        if (l) { memcpy(dst + pos, b[j].data, l); pos += l; }
        else dst[pos++] = *(const uint8_t *) b[j].data;
    }
}

static void copy_run(const copy_job *j)
{
    if (j->kind == 0) {
        memcpy(j->dst, j->src, j->bytes);
    } else if (j->kind == 2) {
        for (size_t i = j->lo; i < j->hi; ++i)
            rc_gather_copy(j->dst + j->poff[i], j->gbuf + j->gfirst[i], j->gfirst[i + 1] - j->gfirst[i]);
    } else {
        for (size_t i = j->lo; i < j->hi; ++i)
            if (j->len[i]) memcpy(j->dst + j->out_off[i], j->src + j->poff[i], j->len[i]);
    }
}

/* A persistent pool of copy_threads - 1 workers (created on first use):
 * creating threads per copy group cost ~1-3 ms per host batch.  One caller
 * at a time uses it; a concurrent caller (several contexts driven from
 * several threads, rc_multi.c) runs its jobs on its own thread. */
static struct {
    pthread_mutex_t mu;
    pthread_cond_t go, done;
    copy_job *jobs;
    int k, next, pending;
} pool = {PTHREAD_MUTEX_INITIALIZER, PTHREAD_COND_INITIALIZER, PTHREAD_COND_INITIALIZER, NULL, 0, 0, 0};
static pthread_mutex_t pool_user = PTHREAD_MUTEX_INITIALIZER;
static pthread_once_t pool_once = PTHREAD_ONCE_INIT;
static int pool_workers;

static void *pool_worker(void *unused)
{
    (void) unused;
    pthread_mutex_lock(&pool.mu);
    for (;;) {
        while (pool.next >= pool.k) pthread_cond_wait(&pool.go, &pool.mu);
        copy_job *j = &pool.jobs[pool.next++];
        pthread_mutex_unlock(&pool.mu);
        copy_run(j);
        pthread_mutex_lock(&pool.mu);
        if (--pool.pending == 0) pthread_cond_signal(&pool.done);
    }
    return NULL;
}

static void pool_start(void)
{
    for (int i = 1; i < rc_host_cfg()->copy_threads; ++i) {
        pthread_t t;
        if (pthread_create(&t, NULL, pool_worker, NULL) != 0) break;
        pthread_detach(t);
        ++pool_workers;
    }
}

static void par_run(copy_job *jobs, int k)
{
    pthread_once(&pool_once, pool_start);
    if (k <= 1 || pool_workers == 0 || pthread_mutex_trylock(&pool_user) != 0) {
        for (int i = 0; i < k; ++i) copy_run(&jobs[i]);
        return;
    }
    pthread_mutex_lock(&pool.mu);
    pool.jobs = jobs;
    pool.next = 1;                  /* job 0 runs here */
    pool.pending = k - 1;
    pool.k = k;
    pthread_cond_broadcast(&pool.go);
    pthread_mutex_unlock(&pool.mu);
    copy_run(&jobs[0]);
    pthread_mutex_lock(&pool.mu);
    while (pool.pending > 0) {
        if (pool.next < pool.k) {   /* help with what is left */
            copy_job *j = &pool.jobs[pool.next++];
            pthread_mutex_unlock(&pool.mu);
            copy_run(j);
            pthread_mutex_lock(&pool.mu);
            --pool.pending;
            continue;
        }
        pthread_cond_wait(&pool.done, &pool.mu);
    }
    pool.k = pool.next = 0;
    pthread_mutex_unlock(&pool.mu);
    pthread_mutex_unlock(&pool_user);
}

static int job_count(uint64_t bytes) { return bytes >= RC_COPY_MIN_BYTES ? rc_host_cfg()->copy_threads : 1; }

void rc_par_memcpy(uint8_t *dst, const uint8_t *src, size_t bytes)
{
    const int k = job_count(bytes);
    copy_job jobs[COPY_THREADS_MAX];
    size_t per = (bytes + k - 1) / k;
    for (int i = 0; i < k; ++i) {
        size_t lo = (size_t) i * per, hi = lo + per < bytes ? lo + per : bytes;
        jobs[i].kind = 0;
        jobs[i].dst = dst + lo; jobs[i].src = src + lo; jobs[i].bytes = hi > lo ? hi - lo : 0;
    }
    par_run(jobs, k);
}

/* packets [lo, hi) of a kind 1 or 2 job in k equal shares */
static void par_packets(copy_job job, size_t lo, size_t hi, int k)
{
    copy_job jobs[COPY_THREADS_MAX];
    const size_t n = hi - lo, per = (n + k - 1) / k;
    for (int i = 0; i < k; ++i) {
        jobs[i] = job;
        jobs[i].lo = lo + ((size_t) i * per < n ? (size_t) i * per : n);
        jobs[i].hi = lo + ((size_t) (i + 1) * per < n ? (size_t) (i + 1) * per : n);
    }
    par_run(jobs, k);
}

void rc_par_scatter(uint8_t *out, const uint64_t *out_off, const uint8_t *packed, const uint64_t *poff,
                    const uint32_t *len, size_t lo, size_t hi, uint64_t bytes)
{
    const copy_job job = {.kind = 1, .dst = out, .src = packed, .out_off = out_off, .poff = poff, .len = len};
    par_packets(job, lo, hi, job_count(bytes));
}

void rc_par_gather(uint8_t *dst, const uint64_t *poff, const ENetBuffer *gbuf, const size_t *gfirst,
                   size_t lo, size_t hi, uint64_t bytes)
{
    const copy_job job = {.kind = 2, .dst = dst, .poff = poff, .gbuf = gbuf, .gfirst = gfirst};
    par_packets(job, lo, hi, job_count(bytes));
}
