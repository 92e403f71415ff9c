// device_buffers_check.cpp -- ekf::DeviceBuffers (openekfmonoslam_amd/csrc/device_buffers.h) against a counting allocator, on the
// host alone: built with -fsanitize=address,undefined and without HIP (tests/test_device_buffers_host.py).  Exits non-zero on a miss.
#include "../../openekfmonoslam_amd/csrc/device_buffers.h"

#include <cstdio>
#include <cstdlib>

static int g_live = 0;     // blocks allocated and not freed
static int g_frees = 0;    // calls of the free fake
static int g_calls = 0;    // allocations asked for since arm()
static int g_fail_at = 0;  // the g_fail_at-th allocation fails (0: none)
static int g_memset_fail = 0; // the next memset fails
static int g_misses = 0;

static hipError_t fake_malloc(void **p, size_t bytes)
{
    if (++g_calls == g_fail_at) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    std::memset(*p, 0xa5, bytes);
    ++g_live;
    return hipSuccess;
}
static hipError_t fake_memset(void *p, int v, size_t bytes)
{
    if (g_memset_fail) {
        g_memset_fail = 0;
        return hipErrorInvalidValue;
    }
    std::memset(p, v, bytes);
    return hipSuccess;
}
static hipError_t fake_free(void *p)
{
    std::free(p);
    --g_live;
    ++g_frees;
    return hipSuccess;
}
static void arm(int fail_at)
{
    g_calls = 0;
    g_fail_at = fail_at;
}

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("MISS %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++g_misses;                                                      \
        }                                                                    \
    } while (0)

int main()
{
    const ekf::DeviceAllocApi api{fake_malloc, fake_memset, fake_free};
    {   // plain alloc: zeroed or not, count 0 -> one element; a failed one leaves the slot null and the live count unchanged
        ekf::DeviceBuffers b(api);
        int *a = nullptr, *z = nullptr, *f = nullptr;
        unsigned char *raw = nullptr;
        void *v = nullptr;
        arm(0);
        CHECK(b.alloc(&a, 7) == hipSuccess && a && g_live == 1);
        for (int i = 0; i < 7; ++i) CHECK(a[i] == 0);
        CHECK(b.alloc(&raw, 3, false) == hipSuccess && raw && raw[0] == 0xa5 && raw[2] == 0xa5);
        CHECK(b.alloc(&z, 0) == hipSuccess && z && z[0] == 0); // (ASan sees the read if less than one int was allocated)
        CHECK(b.alloc_bytes(&v, 16) == hipSuccess && v && g_live == 4);
        arm(1);
        CHECK(b.alloc(&f, 5) == hipErrorOutOfMemory && f == nullptr && g_live == 4);
        arm(0);
        g_memset_fail = 1; // a block whose zeroing fails is not kept
        CHECK(b.alloc(&f, 5) == hipErrorInvalidValue && f == nullptr && g_live == 4);
        // release: frees, forgets, nulls; a null slot and a second release are no-ops
        const int frees = g_frees;
        b.release(&f);
        CHECK(g_frees == frees);
        b.release(&a);
        CHECK(a == nullptr && g_live == 3 && g_frees == frees + 1);
        b.release(&a);
        CHECK(g_live == 3 && g_frees == frees + 1);
        b.release(&v);
        CHECK(v == nullptr && g_live == 2);
        // a released slot can be filled again
        CHECK(b.alloc(&a, 2) == hipSuccess && a && g_live == 3);
    }   // the destructor releases what is still held
    CHECK(g_live == 0);
    {   // release_all with one pointer copied into a second variable (d.pu_tilemap beside pu_tables): exactly one free of it
        ekf::DeviceBuffers b(api);
        void *table = nullptr;
        double *other = nullptr;
        arm(0);
        CHECK(b.alloc_bytes(&table, 64, false) == hipSuccess && b.alloc(&other, 4) == hipSuccess && g_live == 2);
        void *alias = table;
        const int frees = g_frees;
        b.release_all();
        CHECK(g_live == 0 && g_frees == frees + 2 && alias == table);
        b.release_all();
        CHECK(g_live == 0 && g_frees == frees + 2);
    }
    {   // groups
        ekf::DeviceBuffers b(api);
        double *key = nullptr;
        int *all = nullptr, *flag = nullptr;
        long long *recs = nullptr;
        int *before = nullptr;
        arm(0);
        CHECK(b.alloc(&before, 1) == hipSuccess && g_live == 1);
        {   // not committed: the slots are null again and the live count is what it was
            auto g = b.group();
            g.alloc(&key, 8);
            g.alloc(&all, 8);
            CHECK(g.status() == hipSuccess && key && all && g_live == 3);
        }
        CHECK(key == nullptr && all == nullptr && g_live == 1 && before != nullptr);
        {   // committed: survives its scope
            auto g = b.group();
            g.alloc(&key, 8);
            g.alloc(&all, 8, false);
            CHECK(g.commit() == hipSuccess);
        }
        CHECK(key && all && g_live == 3 && key[7] == 0.0);
        b.release(&key);
        b.release(&all);
        CHECK(g_live == 1);
        // the budget's set of four, with the failure at each position: the first status is kept, the allocations behind it do
        // nothing, commit() refuses, and nothing of the set is left
        for (int k = 1; k <= 4; ++k) {
            arm(k);
            {
                auto g = b.group();
                g.alloc(&key, 8);
                g.alloc(&all, 8);
                g.alloc(&flag, 8);
                g.alloc(&recs, 8);
                CHECK(g.status() == hipErrorOutOfMemory);
                CHECK(g_calls == k);       // nothing was asked for behind the failure
                CHECK(g_live == 1 + k - 1); // the ones before it are still there until the group goes
                CHECK(g.commit() == hipErrorOutOfMemory);
            }
            CHECK(key == nullptr && all == nullptr && flag == nullptr && recs == nullptr && g_live == 1);
        }
        arm(0);
        {   // the same set without a failure, and a regrow of it: release, then a new group
            auto g = b.group();
            g.alloc(&key, 8);
            g.alloc(&all, 8);
            g.alloc(&flag, 8);
            g.alloc(&recs, 8);
            CHECK(g.commit() == hipSuccess && g_live == 5);
        }
        b.release(&key);
        b.release(&all);
        arm(2);
        {
            auto g = b.group();
            g.alloc(&key, 16);
            g.alloc(&all, 16);
            CHECK(g.commit() != hipSuccess);
        }
        CHECK(key == nullptr && all == nullptr && flag && recs && g_live == 3);
        arm(0);
    }
    CHECK(g_live == 0);
    if (g_misses) {
        std::printf("device_buffers_check: %d misses\n", g_misses);
        return 1;
    }
    std::printf("device_buffers_check: ok\n");
    return 0;
}
