// device_buffers.h -- the one owner of an engine's device allocations.  Host code only; needs nothing of HIP but hipError_t.
//
// Every device pointer of an engine is allocated and freed here, so "who frees this, and when" has one answer: release() for a
// table that is replaced, release_all() when the engine goes.  The owner records pointer VALUES, not the variables that hold
// them: a pointer copied elsewhere (pu_tables -> d.pu_tilemap, the swap of the two image pyramids) is still owned once.
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cassert>
#include <cstddef>
#include <cstring>
#include <vector>

namespace ekf {

// the allocator behind it: hipMalloc / hipMemset / hipFree in the engine, counting fakes in tests/cpp/device_buffers_check.cpp
struct DeviceAllocApi {
    hipError_t (*malloc_)(void **, size_t);
    hipError_t (*memset_)(void *, int, size_t);
    hipError_t (*free_)(void *);
};

class DeviceBuffers {
public:
    explicit DeviceBuffers(DeviceAllocApi api) : api_(api) {}
    DeviceBuffers(const DeviceBuffers &) = delete;
    DeviceBuffers &operator=(const DeviceBuffers &) = delete;
    ~DeviceBuffers() { release_all(); }

    // *slot (null before the call) = `bytes` bytes, zeroed with a synchronous memset unless zero == false; 0 bytes allocate one.
    // On failure *slot stays null and nothing is held.
    hipError_t alloc_bytes(void **slot, size_t bytes, bool zero = true)
    {
        assert(*slot == nullptr);
        if (bytes == 0) bytes = 1;
        void *p = nullptr;
        hipError_t st = api_.malloc_(&p, bytes);
        if (st != hipSuccess) return st;
        if (zero && (st = api_.memset_(p, 0, bytes)) != hipSuccess) {
            (void)api_.free_(p);
            return st;
        }
        held_.push_back(p);
        *slot = p;
        return hipSuccess;
    }
    template <typename T>
    hipError_t alloc(T **slot, size_t count, bool zero = true)
    {
        assert(*slot == nullptr);
        void *p = nullptr;
        const hipError_t st = alloc_bytes(&p, (count ? count : 1) * sizeof(T), zero);
        *slot = static_cast<T *>(p);
        return st;
    }

    // free what *slot points to, forget it and null the slot; a null slot is a no-op
    template <typename T>
    void release(T **slot)
    {
        free_ptr(*slot);
        *slot = nullptr;
    }
    void release_all()
    {
        for (void *p : held_) (void)api_.free_(p);
        held_.clear();
    }

    // An all-or-nothing set of allocations: unless commit() is reached, the destructor releases what was allocated through the
    // group and nulls those slots.  The first failure is kept in status(), and the allocations behind it do nothing.
    class Group {
    public:
        explicit Group(DeviceBuffers &bufs) : bufs_(bufs) {}
        Group(const Group &) = delete;
        Group &operator=(const Group &) = delete;
        ~Group()
        {
            if (committed_) return;
            for (void *slot : slots_) { // (the slots have different pointer types: read and null them as bytes)
                void *p = nullptr;
                std::memcpy(&p, slot, sizeof p);
                bufs_.free_ptr(p);
                std::memset(slot, 0, sizeof p);
            }
        }
        void alloc_bytes(void **slot, size_t bytes, bool zero = true)
        {
            if (st_ == hipSuccess && (st_ = bufs_.alloc_bytes(slot, bytes, zero)) == hipSuccess) slots_.push_back(slot);
        }
        template <typename T>
        void alloc(T **slot, size_t count, bool zero = true)
        {
            if (st_ == hipSuccess && (st_ = bufs_.alloc(slot, count, zero)) == hipSuccess) slots_.push_back(slot);
        }
        hipError_t status() const { return st_; }
        // keeps the allocations if every one of them succeeded; returns status()
        hipError_t commit()
        {
            committed_ = st_ == hipSuccess;
            return st_;
        }

    private:
        DeviceBuffers &bufs_;
        std::vector<void *> slots_; // addresses of the slots filled through this group
        hipError_t st_ = hipSuccess;
        bool committed_ = false;
    };
    Group group() { return Group(*this); }

private:
    void free_ptr(void *p)
    {
        if (!p) return;
        auto it = std::find(held_.begin(), held_.end(), p);
        assert(it != held_.end());
        if (it == held_.end()) return; // not ours (or freed already): never a second free
        *it = held_.back();
        held_.pop_back();
        (void)api_.free_(p);
    }

    DeviceAllocApi api_;
    std::vector<void *> held_;
};

} // namespace ekf
