// alll_rt_util.h -- error reporting shared by the three device runtimes (alll_runtime.cpp,
// alll_batch_runtime.cpp, alll_group_runtime.cpp): the message goes to the calling thread's
// alll_last_error() string, the code is returned.  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "alll.h"

extern "C" void alll_internal_set_error(const char* msg);  // (alll_runtime.cpp)

namespace alll {

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    alll_internal_set_error(buf);
    return code;
}

}  // namespace alll

#define HIP_TRY(expr)                                                                    \
    do {                                                                                 \
        hipError_t _e = (expr);                                                          \
        if (_e != hipSuccess)                                                            \
            return ::alll::fail(ALLL_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                             \
    } while (0)
