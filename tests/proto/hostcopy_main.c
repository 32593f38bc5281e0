/*
 * hostcopy_main.c -- the host shim's copy threads (enet_amd/csrc/rc_hostcopy.c)
 * against serial loops, on the CPU.  Built with the sanitizers by
 * tests/test_hostcopy.py; exit status 0: all checks passed.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rc_host_internal.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(void)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) (rng_state >> 33);
}

static uint8_t *random_bytes(size_t n)
{
    uint8_t *p = (uint8_t *) malloc(n ? n : 1);
    CHECK(p);
    for (size_t i = 0; i + 4 <= n; i += 4) { const uint32_t r = rnd(); memcpy(p + i, &r, 4); }
    for (size_t i = n & ~(size_t) 3; i < n; ++i) p[i] = (uint8_t) rnd();
    return p;
}

static void check_memcpy(size_t bytes)
{
    uint8_t *src = random_bytes(bytes), *dst = (uint8_t *) malloc(bytes + 2);
    CHECK(dst);
    memset(dst, 0xEE, bytes + 2);
    rc_par_memcpy(dst + 1, src, bytes);
    CHECK(dst[0] == 0xEE && dst[bytes + 1] == 0xEE);
    CHECK(memcmp(dst + 1, src, bytes) == 0);
    free(src);
    free(dst);
}

/* 5000 ragged packets of 0-3000 B (every 50th empty) packed back to back,
 * scattered into gapped slots; the bytes between the slots stay as they were */
typedef struct {
    size_t n;
    uint32_t *len;
    uint64_t *poff, *ooff;
    uint8_t *packed, *out, *want;
    size_t packed_bytes, out_bytes;
} scatter_case;

static void scatter_make(scatter_case *s)
{
    s->n = 5000;
    s->len = (uint32_t *) malloc(s->n * sizeof(uint32_t));
    s->poff = (uint64_t *) malloc(s->n * sizeof(uint64_t));
    s->ooff = (uint64_t *) malloc(s->n * sizeof(uint64_t));
    CHECK(s->len && s->poff && s->ooff);
    uint64_t pa = 0, oa = 3;
    for (size_t i = 0; i < s->n; ++i) {
        s->len[i] = i % 50 == 0 ? 0 : rnd() % 3001;
        s->poff[i] = pa;
        s->ooff[i] = oa;
        pa += s->len[i];
        oa += s->len[i] + 1 + rnd() % 9;
    }
    CHECK(pa > RC_COPY_MIN_BYTES);          /* the pool runs */
    s->packed_bytes = pa;
    s->out_bytes = oa;
    s->packed = random_bytes(pa);
    s->out = (uint8_t *) malloc(oa);
    s->want = (uint8_t *) malloc(oa);
    CHECK(s->out && s->want);
    memset(s->out, 0xA5, oa);
    memset(s->want, 0xA5, oa);
    for (size_t i = 0; i < s->n; ++i) memcpy(s->want + s->ooff[i], s->packed + s->poff[i], s->len[i]);
}

static void *scatter_run(void *p)
{
    scatter_case *s = (scatter_case *) p;
    rc_par_scatter(s->out, s->ooff, s->packed, s->poff, s->len, 0, s->n, s->packed_bytes);
    return NULL;
}

static void scatter_check_free(scatter_case *s)
{
    CHECK(memcmp(s->out, s->want, s->out_bytes) == 0);
    free(s->len); free(s->poff); free(s->ooff); free(s->packed); free(s->out); free(s->want);
}

/* gather lists as compress.c:260-285 walks them: an empty first buffer yields
 * nothing, an empty later buffer its data[0] (the phantom byte) */
static void check_gather(void)
{
    enum { N = 6000, BUFS = 4, MAXLEN = 1400, POOL = 1 << 20 };
    uint8_t *pool = random_bytes(POOL);
    ENetBuffer *bufs = (ENetBuffer *) malloc(sizeof(ENetBuffer) * N * BUFS);
    size_t *first = (size_t *) malloc(sizeof(size_t) * (N + 1));
    uint64_t *poff = (uint64_t *) malloc(sizeof(uint64_t) * N);
    CHECK(bufs && first && poff);
    size_t nb = 0, total = 0;
    for (size_t i = 0; i < N; ++i) {
        first[i] = nb;
        const size_t k = i % 97 == 5 ? 0 : 1 + rnd() % BUFS;       /* some packets have no buffer */
        for (size_t j = 0; j < k; ++j, ++nb) {
            bufs[nb].data = pool + rnd() % (POOL - MAXLEN);
            bufs[nb].dataLength = 1 + rnd() % MAXLEN;
            if (j == 0 && i % 7 == 1) bufs[nb].dataLength = 0;      /* an empty first buffer */
            if (j > 0 && i % 5 == 2) bufs[nb].dataLength = 0;       /* an empty later buffer */
        }
        poff[i] = total;
        total += rc_gather_len(bufs + first[i], k);
    }
    first[N] = nb;
    CHECK(total > RC_COPY_MIN_BYTES);
    uint8_t *want = (uint8_t *) malloc(total), *got = (uint8_t *) malloc(total);
    CHECK(want && got);
    size_t pos = 0;
    for (size_t i = 0; i < N; ++i) {
        CHECK(pos == poff[i]);
        for (size_t b = first[i]; b < first[i + 1]; ++b) {
            const uint8_t *d = (const uint8_t *) bufs[b].data;
            if (bufs[b].dataLength) { memcpy(want + pos, d, bufs[b].dataLength); pos += bufs[b].dataLength; }
            else if (b > first[i]) want[pos++] = d[0];
        }
    }
    CHECK(pos == total);                    /* rc_gather_len agrees with the flattened bytes */
    memset(got, 0, total);
    rc_par_gather(got, poff, bufs, first, 0, N, total);
    CHECK(memcmp(got, want, total) == 0);
    free(pool); free(bufs); free(first); free(poff); free(want); free(got);
}

int main(void)
{
    check_memcpy((9u << 20) + 3);           /* above RC_COPY_MIN_BYTES: on the pool */
    check_memcpy(100);
    scatter_case one;
    scatter_make(&one);
    scatter_run(&one);
    scatter_check_free(&one);
    check_gather();
    /* two callers at once: one of them finds the pool taken and runs its jobs itself */
    scatter_case a, b;
    pthread_t ta, tb;
    scatter_make(&a);
    scatter_make(&b);
    CHECK(pthread_create(&ta, NULL, scatter_run, &a) == 0);
    CHECK(pthread_create(&tb, NULL, scatter_run, &b) == 0);
    pthread_join(ta, NULL);
    pthread_join(tb, NULL);
    scatter_check_free(&a);
    scatter_check_free(&b);
    puts("hostcopy ok");
    return 0;
}
