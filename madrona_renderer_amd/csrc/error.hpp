// The failure text of the calling thread (mrx_last_error): one per thread for the whole library, whichever unit set it.
#pragma once

#include <string>

#pragma GCC visibility push(hidden)

inline thread_local std::string g_err;

inline int fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}

#pragma GCC visibility pop
