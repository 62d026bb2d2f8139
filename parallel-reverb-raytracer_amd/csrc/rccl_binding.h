// rccl_binding.h — RCCL bound at run time for csrc/multi.hip's one all-reduce: librccl.so is loaded on first use, so that the library
// links and runs without it (the peer-copy sum of multi.hip takes over).
#pragma once

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <cstdlib>

// ---- the four RCCL entry points used, bound at run time (prototypes: /opt/rocm/include/rccl/rccl.h:236, :260, :339, :611, :919) ----
typedef struct ncclComm * ncclComm_t;
struct Rccl {
    void * lib = nullptr;
    int (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    int (*CommDestroy)(ncclComm_t) = nullptr;
    const char * (*GetErrorString)(int) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    bool ok() const { return CommInitAll && CommDestroy && GetErrorString && AllReduce && GroupStart && GroupEnd; }
};
const int kNcclFloat = 7, kNcclSum = 0;       // rccl.h:466, :448

static Rccl & rccl()           // (internal: one binding per translation unit that asks)
{
    static Rccl r = [] {
        Rccl x;
        const char * names[] = {getenv("RVB_RCCL_LIB"), "librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
        for (const char * n : names) {
            if (!n) continue;
            x.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (x.lib) break;
        }
        if (x.lib) {
            x.CommInitAll = reinterpret_cast<int (*)(ncclComm_t *, int, const int *)>(dlsym(x.lib, "ncclCommInitAll"));
            x.CommDestroy = reinterpret_cast<int (*)(ncclComm_t)>(dlsym(x.lib, "ncclCommDestroy"));
            x.GetErrorString = reinterpret_cast<const char * (*)(int)>(dlsym(x.lib, "ncclGetErrorString"));
            x.AllReduce = reinterpret_cast<int (*)(const void *, void *, size_t, int, int, ncclComm_t, hipStream_t)>(dlsym(x.lib, "ncclAllReduce"));
            x.GroupStart = reinterpret_cast<int (*)()>(dlsym(x.lib, "ncclGroupStart"));
            x.GroupEnd = reinterpret_cast<int (*)()>(dlsym(x.lib, "ncclGroupEnd"));
        }
        return x;
    }();
    return r;
}
