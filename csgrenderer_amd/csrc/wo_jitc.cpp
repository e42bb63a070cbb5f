// wo_jitc: compiles one generated specialised-kernel source with the system ROCm's
// hiprtc, in a process of its own.  The library runs it (jit_code.cpp jitc_compile)
// when the hiprtc serving the library's process is another ROCm's -- a
// process that imported torch first runs on torch's bundled HIP runtime, hiprtc and
// comgr, whose older compiler spills where the system's does not (DESIGN.md §0 round 6
// item 2).  Links only hiprtc (no GPU is touched).
//
//   wo_jitc <source file> <code object out> [hiprtc options ...]   exit 0: compiled
#include <stdio.h>

#include "jit_hiprtc.h"

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: wo_jitc <source> <out> [options...]\n");
        return 2;
    }
    std::string src;
    {
        FILE* f = fopen(argv[1], "rb");
        if (!f) return 3;
        char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) src.append(buf, n);
        fclose(f);
    }
    std::vector<char> code;
    hiprtcResult rc;
    std::string log;
    if (const int st = wo_hiprtc_compile(src.c_str(), std::vector<const char*>(argv + 3, argv + argc), code, &rc, &log)) {
        if (st == WO_RTC_FAILED) fprintf(stderr, "%.2000s\n", log.c_str());
        return st;  // 4: no program, 5: the compile failed
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 6;
    const bool ok = fwrite(code.data(), 1, code.size(), o) == code.size();
    return fclose(o) == 0 && ok ? 0 : 7;
}
