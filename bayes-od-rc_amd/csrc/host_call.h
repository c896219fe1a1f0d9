// Host-side plumbing shared by the stateless evaluation drivers (pdq_kernels.hip, score_kernels.hip): the error message of a call
// and the device allocations it frees on every exit path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

struct Err {
    char* buf; size_t cap;
    int fail(int status, const char* fmt, ...) {
        va_list ap; va_start(ap, fmt); vsnprintf(buf, cap, fmt, ap); va_end(ap);
        return status;
    }
};

struct DevArena {           // device allocations of one call, freed on every exit path
    std::vector<void*> ptrs;
    ~DevArena() { for (void* p : ptrs) hipFree(p); }
    template <typename T> hipError_t alloc(T** p, size_t n) {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(n * sizeof(T), 256));
        if (e == hipSuccess) ptrs.push_back(q);
        *p = reinterpret_cast<T*>(q);
        return e;
    }
    void release() { for (void* p : ptrs) hipFree(p); ptrs.clear(); }
};
