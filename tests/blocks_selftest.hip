// blocks_selftest.hip -- the rules of hs_block and of the unit table (csrc/hs_blocks.h) on the CPU, with no GPU: the four allocation
// calls are counting, malloc-backed stand-ins (HS_BLOCKS_SELFTEST), one of which can be told to fail.  A stand-alone program: it
// prints "ok" and returns 0, or names the line that failed.  tests/test_blocks_selftest.py compiles and runs it.
#include <hip/hip_runtime.h>
#include <map>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

static std::map<void *, int> st_live;      // pointer -> 0 device, 1 pinned host
static long st_allocs, st_frees, st_bad_frees, st_fail_in = -1;   // st_fail_in: the allocation, counted from now, that fails

static hipError_t st_alloc(void **p, size_t bytes, int host)
{
    if (st_fail_in == 0) { st_fail_in = -1; return hipErrorOutOfMemory; }
    if (st_fail_in > 0) st_fail_in--;
    *p = malloc(bytes ? bytes : 1);
    st_live[*p] = host;
    st_allocs++;
    return hipSuccess;
}
static hipError_t st_release(void *p, int host)
{
    auto it = st_live.find(p);
    if (it == st_live.end() || it->second != host) { st_bad_frees++; return hipErrorInvalidValue; }   // (twice, or by the other kind's call)
    st_live.erase(it);
    free(p);
    st_frees++;
    return hipSuccess;
}
static hipError_t selftest_malloc(void **p, size_t bytes) { return st_alloc(p, bytes, 0); }
static hipError_t selftest_host_malloc(void **p, size_t bytes, unsigned) { return st_alloc(p, bytes, 1); }
static hipError_t selftest_free(void *p) { return st_release(p, 0); }
static hipError_t selftest_host_free(void *p) { return st_release(p, 1); }

#define HS_BLOCKS_SELFTEST 1
#include "hs_blocks.h"

std::atomic<int64_t> hs_live_blocks{0}, hs_live_bytes{0};
static char st_error[512];
void slamhip_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(st_error, sizeof(st_error), fmt, ap);
    va_end(ap);
}

#define CHECK(c) do { if (!(c)) { printf("blocks_selftest.hip:%d: %s\n", __LINE__, #c); return 1; } } while (0)
static bool live(int64_t blocks, int64_t bytes) { return hs_live_blocks.load() == blocks && hs_live_bytes.load() == bytes && (int64_t)st_live.size() == blocks; }

// two of the units of slamhip_hs, as this program defines them
struct hs_nav { hs_block<uint32_t, HS_MEM_DEVICE> a; hs_block<unsigned char, HS_MEM_PINNED> b; hs_block<int, HS_MEM_PINNED_VISIBLE> c[2]; };
struct hs_view { hs_block<float, HS_MEM_DEVICE> a; };

static int32_t early_return(bool leave)
{
    hs_block<float, HS_MEM_DEVICE> t;
    SH_TRY(t.grow(40, "selftest"));
    if (leave) SH_FAIL(SLAMHIP_ERR_INVALID, "left early");
    return SLAMHIP_OK;
}

int main()
{
    {
        // grow, then reuse while the block is large enough
        hs_block<uint32_t, HS_MEM_DEVICE> d;
        CHECK(d.p == nullptr && d.cap == 0 && live(0, 0));
        CHECK(d.grow(0, "selftest") == SLAMHIP_OK && d.p == nullptr && st_allocs == 0);
        CHECK(d.grow(100, "selftest") == SLAMHIP_OK && d.p && d.cap == 100 && live(1, 100));
        uint32_t *first = d;
        CHECK(d.grow(100, "selftest") == SLAMHIP_OK && d.grow(7, "selftest") == SLAMHIP_OK && d.p == first && d.cap == 100 && st_allocs == 1 && st_frees == 0);
        // grow larger: the old block is freed exactly once
        CHECK(d.grow(101, "selftest") == SLAMHIP_OK && d.cap == 101 && st_allocs == 2 && st_frees == 1 && live(1, 101));
        // a failed grow leaves the block empty and the counters right
        st_fail_in = 0;
        CHECK(d.grow(500, "selftest") == SLAMHIP_ERR_NOMEM && d.p == nullptr && d.cap == 0 && st_frees == 2 && live(0, 0));
        CHECK(strcmp(st_error, "selftest: allocation of 500 bytes of device memory failed") == 0);
        hs_block<unsigned char, HS_MEM_PINNED> h;
        st_fail_in = 0;
        CHECK(h.grow(9, "selftest") == SLAMHIP_ERR_NOMEM && strcmp(st_error, "selftest: allocation of 9 bytes of pinned host memory failed") == 0 && live(0, 0));
        CHECK(d.grow(8, "selftest") == SLAMHIP_OK && h.grow(16, "selftest") == SLAMHIP_OK && live(2, 24));
        CHECK(st_live[d.p] == 0 && st_live[h.p] == 1);                     // each kind by its own call
        // swap moves ownership
        hs_block<uint32_t, HS_MEM_DEVICE> e;
        uint32_t *was = d;
        e.swap(d);
        CHECK(d.p == nullptr && d.cap == 0 && e.p == was && e.cap == 8 && live(2, 24));
        {
            hs_block<uint32_t, HS_MEM_DEVICE> bigger;
            CHECK(bigger.grow(64, "selftest") == SLAMHIP_OK && live(3, 88));
            e.swap(bigger);                                                // (the smaller block goes with `bigger`)
        }
        CHECK(e.cap == 64 && live(2, 80));
        e.release(); e.release();
        CHECK(e.p == nullptr && live(1, 16) && st_bad_frees == 0);
    }
    CHECK(live(0, 0));                                                      // (h went with its scope)
    // a destructor in scope frees the block on an early return
    long frees = st_frees;
    CHECK(early_return(true) == SLAMHIP_ERR_INVALID && st_frees == frees + 1 && live(0, 0));
    CHECK(early_return(false) == SLAMHIP_OK && st_frees == frees + 2 && live(0, 0));

    // a struct of blocks deleted through the unit table frees all of them; a slot is recorded once
    slamhip_hs *hs = (slamhip_hs *)calloc(1, sizeof(slamhip_hs));
    CHECK(hs);
    CHECK(hs_unit<&slamhip_hs::nav>(hs) == SLAMHIP_OK && hs->nav && hs->n_units == 1);
    hs_nav *nav = hs->nav;
    CHECK(hs_unit<&slamhip_hs::nav>(hs) == SLAMHIP_OK && hs->nav == nav && hs->n_units == 1);
    CHECK(nav->a.grow(12, "selftest") == SLAMHIP_OK && nav->b.grow(20, "selftest") == SLAMHIP_OK && nav->c[0].grow(4, "selftest") == SLAMHIP_OK &&
          nav->c[1].grow(8, "selftest") == SLAMHIP_OK && live(4, 44));
    CHECK(hs_unit<&slamhip_hs::vw>(hs) == SLAMHIP_OK && hs->n_units == 2 && hs->vw->a.grow(16, "selftest") == SLAMHIP_OK && live(5, 60));
    hs_unit_drop<&slamhip_hs::nav>(hs);                                    // what a *_clear entry point does
    CHECK(hs->nav == nullptr && hs->n_units == 2 && live(1, 16));
    hs_unit_drop<&slamhip_hs::nav>(hs);                                    // (a second clear finds nothing)
    CHECK(hs->nav == nullptr && live(1, 16) && st_bad_frees == 0);
    for (int k = 0; k < 2 * HS_MAX_UNITS; k++) {                           // drop and re-create, more often than the table has entries
        CHECK(hs_unit<&slamhip_hs::nav>(hs) == SLAMHIP_OK && hs->n_units == 2 && hs->nav->b.grow(32, "selftest") == SLAMHIP_OK && live(2, 48));
        hs_unit_drop<&slamhip_hs::nav>(hs);
    }
    CHECK(hs_unit<&slamhip_hs::nav>(hs) == SLAMHIP_OK && hs->nav->a.grow(24, "selftest") == SLAMHIP_OK && live(2, 40));
    hs_units_drop_all(hs);                                                 // slamhip_hs_destroy's walk
    CHECK(hs->nav == nullptr && hs->vw == nullptr && hs->n_units == 0 && live(0, 0));
    free(hs);

    CHECK(hs_live_blocks.load() == 0 && hs_live_bytes.load() == 0 && st_live.empty());
    CHECK(st_allocs == st_frees && st_allocs > 0 && st_bad_frees == 0);
    printf("ok: %ld allocations, %ld frees\n", st_allocs, st_frees);
    return 0;
}
