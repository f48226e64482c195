// hip_host.hpp — what the translation units of the C ABI share on the host: the error return, the
// HIP status check and a device allocation that grows on demand.
#pragma once

#include <hip/hip_runtime.h>

#include <string>

#include "../../../include/mpccbf.h"
#include "errors.hpp"

namespace mpccbf {

inline int fail(int code, const std::string& msg) { return set_error(code, msg); }

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail(MPCCBF_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
    } while (0)

// A device allocation that grows on demand and is freed with its owner. After a failed growth it
// is empty (bytes == 0), so the next call allocates again.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    // at least `need` bytes (a buffer that has to grow is reallocated: its contents are gone)
    hipError_t reserve(size_t need) {
        if (need <= bytes) return hipSuccess;
        release();
        const hipError_t e = hipMalloc(&p, need);
        if (e == hipSuccess) bytes = need; else p = nullptr;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
};

}  // namespace mpccbf
