// jit_hiprtc.h -- one hiprtc compile of a generated specialised-kernel source against
// the embedded device headers: the library's in-process compile (jit_code.cpp) and the
// helper process (wo_jitc.cpp) are this one function.  Host only; no GPU is touched.
#ifndef WOLOLO_JIT_HIPRTC_H
#define WOLOLO_JIT_HIPRTC_H

#include <hip/hiprtc.h>

#include <string>
#include <vector>

#include "jit_sources.inc"

// 0 and the code object; WO_RTC_NO_PROGRAM; or WO_RTC_FAILED with hiprtc's result in
// *rc and the compiler's log in *log.  (The values are wo_jitc's exit codes.)
enum { WO_RTC_NO_PROGRAM = 4, WO_RTC_FAILED = 5 };
static inline int wo_hiprtc_compile(const char* src, const std::vector<const char*>& opts, std::vector<char>& code,
                                    hiprtcResult* rc, std::string* log) {
    const char* hdr_src[] = {kEmbed_wo_device_common_h, kEmbed_wo_scene_h};
    const char* hdr_names[] = {"wo_device_common.h", "wololo/wo_scene.h"};
    hiprtcProgram p;
    if (hiprtcCreateProgram(&p, src, "wo_scene_jit.hip", 2, hdr_src, hdr_names) != HIPRTC_SUCCESS)
        return WO_RTC_NO_PROGRAM;
    *rc = hiprtcCompileProgram(p, (int)opts.size(), const_cast<const char**>(opts.data()));
    if (*rc != HIPRTC_SUCCESS) {
        size_t ls = 0;
        hiprtcGetProgramLogSize(p, &ls);
        log->assign(ls + 1, '\0');
        hiprtcGetProgramLog(p, &(*log)[0]);
        hiprtcDestroyProgram(&p);
        return WO_RTC_FAILED;
    }
    size_t cs = 0;
    hiprtcGetCodeSize(p, &cs);
    code.resize(cs);
    hiprtcGetCode(p, code.data());
    hiprtcDestroyProgram(&p);
    return 0;
}

#endif  // WOLOLO_JIT_HIPRTC_H
