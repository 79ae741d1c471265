// The host prover's error text: one buffer per thread, written by fail() and
// read back by zkgpu_stark_last_error in the thread that made the failing call.
// Shared by every unit of libzkgpu_stark and by the communicators' checks.
#pragma once
#include <stdarg.h>
#include <stdio.h>

#include <string>

#include "../../include/zkgpu.h"

namespace zkgpu_host {

inline thread_local char g_err[512] = "";
inline int fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return -1;
}
// the message of the last fail() on this thread (e.g. a communicator's, before
// the prover's own wraps it)
inline std::string last_error_text() { return g_err; }

}  // namespace zkgpu_host

// a libzkgpu call inside namespace zkgpu_host: its failure is the caller's, with the library's text
#define CK(x)                                                                                                  \
    do {                                                                                                       \
        int _rc = (x);                                                                                         \
        if (_rc) return fail("%s: %s (%s:%d)", #x, zkgpu_last_error(), __FILE__, __LINE__);                   \
    } while (0)
