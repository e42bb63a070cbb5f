// jit_code.h -- the specialised kernels' code objects (jit_code.cpp, host only): from a
// generated source (scene_jit.c) to the bytes hipModuleLoadData takes, through the
// process cache, the disk cache (jit_cache.c) and a compiler.  Internal, C++; the C
// entry points built on it are declared in wo_dev.h and renderer_ext.h.
#ifndef WOLOLO_JIT_CODE_H
#define WOLOLO_JIT_CODE_H

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "wo_dev.h"

namespace wojit {

// `helper` everywhere: the compiler.  "" = the hiprtc serving this process, else the
// path of a wo_jitc to run; the library passes jitc_path().
const std::string& jitc_path();

struct JitCode {
    std::vector<char> code;  // the code object
    std::string key;         // SHA-256 (hex) of everything it depends on, the compiler included
    int origin = -1;         // 0 the process cache, 1 the disk cache, 2 compiled now
    double seconds = 0.0;    // what getting it took
};

// `count`: the counting variant (executed-work counters, wo_dev_count_work)
std::string jit_key(const char* src, const std::string& arch, bool count = false,
                    const std::string& helper = jitc_path());
// The object of `src`: looked up under the helper's key, else compiled by the helper and
// stored under that key; without a helper, or when the helper yields no object, the same
// with this process's hiprtc and its key.  0, or -1 with the compiler's message.
int jit_code(const char* src, const std::string& arch, bool count, JitCode* out, char* err, size_t errlen,
             const std::string& helper = jitc_path());
// `key`'s object from the process cache (origin 0) or the disk cache (1, and promoted to
// the process cache); -1: in neither.
int jit_lookup(const std::string& key, std::vector<char>* code);
// the process cache alone: the 8 most recently put or got objects
void jit_cache_put(const std::string& key, const std::vector<char>& code);
bool jit_cache_get(const std::string& key, std::vector<char>* code);
// wo_jit_job_start (wo_dev.h) for a target
WoJitJob* jit_job_start(const char* src, const std::string& arch);

// The group (LDS) and private (scratch per lane) segment sizes of kernel `name` as the
// code object of n bytes states them; false if it is not such an ELF.
bool kd_segment_sizes(const void* code, size_t n, const char* name, uint32_t* group, uint32_t* priv);

}  // namespace wojit

#endif  // WOLOLO_JIT_CODE_H
