// jit_code.cpp -- the specialised kernels' code-object pipeline (jit_code.h): the process
// cache in front of the disk cache (jit_cache.c), the key, the two compilers (this
// process's hiprtc and the wo_jitc helper), the kernel-descriptor reader and the
// background compiles.  Host only: no kernel, no device, no HIP module -- loading an
// object is trace_kernels.hip's.  tests/host/jit_code_main.cpp drives it under sanitizers.
#include <hip/hip_runtime_api.h>

#include <dlfcn.h>
#include <limits.h>
#include <spawn.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/wait.h>
#include <unistd.h>

#include <array>
#include <atomic>
#include <chrono>
#include <mutex>
#include <thread>
#include <unordered_map>

#include "jit_code.h"
#include "jit_hiprtc.h"

extern "C" char** environ;

namespace wojit {

// Process-wide cache of compiled code objects (the same scene compiled once per
// process, loaded on every rank), in front of the on-disk cache (jit_cache.c)
// shared by processes.  Bounded: the least recently used entries go beyond
// kJitCacheEntries (an interactive session that edits the scene would otherwise
// keep every version's object, megabytes each; the disk cache still has them).
struct JitEntry {
    std::vector<char> code;
    uint64_t used;
};
static const size_t kJitCacheEntries = 8;
// The process cache and its lock live on the heap and are never destroyed: a
// background compile still running when the process exits (a renderer never
// closed) then touches no destroyed static.
static std::mutex& g_jit_mu = *new std::mutex;
static uint64_t g_jit_tick;
static std::unordered_map<std::string, JitEntry>& jit_cache() {
    static auto* m = new std::unordered_map<std::string, JitEntry>;
    return *m;
}

void jit_cache_put(const std::string& key, const std::vector<char>& code) {
    std::lock_guard<std::mutex> lock(g_jit_mu);
    auto& m = jit_cache();
    m[key] = JitEntry{code, ++g_jit_tick};
    while (m.size() > kJitCacheEntries) {
        auto old = m.begin();
        for (auto it = m.begin(); it != m.end(); ++it)
            if (it->second.used < old->second.used) old = it;
        m.erase(old);
    }
}

bool jit_cache_get(const std::string& key, std::vector<char>* code) {
    std::lock_guard<std::mutex> lock(g_jit_mu);
    auto it = jit_cache().find(key);
    if (it == jit_cache().end()) return false;
    it->second.used = ++g_jit_tick;
    *code = it->second.code;
    return true;
}

int jit_lookup(const std::string& key, std::vector<char>* code) {
    if (jit_cache_get(key, code)) return 0;
    void* buf = nullptr;
    size_t n = 0;
    if (wo_jit_disk_load(key.c_str(), &buf, &n) != 0) return -1;
    code->assign((char*)buf, (char*)buf + n);
    free(buf);
    jit_cache_put(key, *code);
    return 1;
}

// Extra hiprtc options from WOLOLO_JIT_FLAGS (space separated), e.g.
// "-DWO_WINDOW=2 -DWO_JIT_MIN_WAVES=4" -- a tuning knob; part of the cache key.
static std::vector<std::string> jit_extra_flags() {
    std::vector<std::string> out;
    const char* e = getenv("WOLOLO_JIT_FLAGS");
    if (!e) return out;
    std::string s(e), cur;
    for (char c : s) {
        if (c == ' ') {
            if (!cur.empty()) out.push_back(cur);
            cur.clear();
        } else {
            cur.push_back(c);
        }
    }
    if (!cur.empty()) out.push_back(cur);
    return out;
}

static std::vector<std::string> jit_options(const std::string& arch, bool count) {
    // no SLP vectorisation: its packed fp32 pairs need register moves to form and
    // shorten no dependent chain (csg32 4.14 -> 4.05 ms, csg256 balanced 12.50 -> 12.08);
    // WOLOLO_JIT_FLAGS=-fslp-vectorize turns it back on
    std::vector<std::string> opts = {"--offload-arch=" + arch, "-O3", "-ffp-contract=off", "-std=c++17",
                                     "-fno-slp-vectorize"};
    for (const std::string& f : jit_extra_flags()) opts.push_back(f);
    if (count) opts.push_back("-DWO_COUNT_WORK=1");
    return opts;
}

// The compiler process (wo_jitc, next to this library): used when the hiprtc that
// serves this process is not the system ROCm's -- a process that imported torch first
// runs the library on torch's bundled HIP runtime, hiprtc and comgr (the sonames are
// shared), and that older compiler spilled csg32_nested's kernel (12 B per lane, 3 %
// slower).  wo_jitc links only the system hiprtc, in a
// process of its own.  "" = compile in this process (the system hiprtc serves it, the
// helper is missing, or WOLOLO_JITC=0).
const std::string& jitc_path() {
    static const std::string path = []() -> std::string {
        const char* env = getenv("WOLOLO_JITC");
        if (env && *env == '0') return std::string();
        Dl_info di;
        char rp[PATH_MAX], rr[PATH_MAX];
        const char* root = getenv("ROCM_PATH");
        if (dladdr((void*)&hiprtcCompileProgram, &di) && di.dli_fname && realpath(di.dli_fname, rp) &&
            realpath(root && *root ? root : "/opt/rocm", rr) && strncmp(rp, rr, strlen(rr)) == 0)
            return std::string();  // the system hiprtc already
        if (!dladdr((void*)&jitc_path, &di) || !di.dli_fname) return std::string();
        std::string lib(di.dli_fname);
        const size_t slash = lib.rfind('/');
        std::string p = (slash == std::string::npos ? std::string(".") : lib.substr(0, slash)) + "/wo_jitc";
        return access(p.c_str(), X_OK) == 0 ? p : std::string();
    }();
    return path;
}

// One compile through the helper: the source and the code object through a private
// temporary directory.  False: no object (its diagnostics went to stderr).
static bool jitc_compile(const std::string& helper, const char* src, const std::vector<std::string>& opts,
                         std::vector<char>& code) {
    const char* td = getenv("TMPDIR");
    std::string dir = std::string(td && *td ? td : "/tmp") + "/wojitc.XXXXXX";
    if (!mkdtemp(&dir[0])) return false;
    const std::string in = dir + "/k.hip", out = dir + "/k.co";
    bool ok = false;
    if (FILE* f = fopen(in.c_str(), "wb")) {
        const size_t n = strlen(src);
        ok = fwrite(src, 1, n, f) == n;
        ok = (fclose(f) == 0) && ok;
    }
    if (ok) {
        std::vector<char*> argv;
        argv.push_back(const_cast<char*>(helper.c_str()));
        argv.push_back(const_cast<char*>(in.c_str()));
        argv.push_back(const_cast<char*>(out.c_str()));
        for (const std::string& o : opts) argv.push_back(const_cast<char*>(o.c_str()));
        argv.push_back(nullptr);
        pid_t pid;
        int st = 0;
        ok = posix_spawn(&pid, helper.c_str(), nullptr, nullptr, argv.data(), environ) == 0 &&
             waitpid(pid, &st, 0) == pid && WIFEXITED(st) && WEXITSTATUS(st) == 0;
    }
    if (ok) {
        ok = false;
        if (FILE* f = fopen(out.c_str(), "rb")) {
            std::vector<char> buf;
            char tmp[65536];
            size_t n;
            while ((n = fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + n);
            fclose(f);
            ok = buf.size() >= 4 && memcmp(buf.data(), "\x7f" "ELF", 4) == 0;
            if (ok) code.swap(buf);
        }
    }
    (void)unlink(in.c_str());
    (void)unlink(out.c_str());
    (void)rmdir(dir.c_str());
    return ok;
}

// One compile by `helper`, or by this process's hiprtc ("", which fills `err`).
static int jit_compile(const std::string& helper, const char* src, const std::string& arch, bool count,
                       std::vector<char>& code, char* err, size_t errlen) {
    const std::vector<std::string> opt_s = jit_options(arch, count);
    if (!helper.empty()) return jitc_compile(helper, src, opt_s, code) ? 0 : -1;
    std::vector<const char*> opts;
    for (const std::string& o : opt_s) opts.push_back(o.c_str());
    hiprtcResult rc;
    std::string log;
    const int st = wo_hiprtc_compile(src, opts, code, &rc, &log);
    if (st == WO_RTC_FAILED)
        snprintf(err, errlen, "hiprtc: %s: %.400s", hiprtcGetErrorString(rc), log.c_str());
    else if (st)
        snprintf(err, errlen, "hiprtcCreateProgram failed");
    return st ? -1 : 0;
}

// The compilers to try, in order: the helper if there is one, then this process's.  An
// object is cached under the key of the compiler that built it, so a failed helper never
// puts the in-process compiler's object under the helper's key.
static std::vector<std::string> compilers(const std::string& helper) {
    return helper.empty() ? std::vector<std::string>{helper} : std::vector<std::string>{helper, std::string()};
}

// SHA-256 over everything the code object depends on: a format tag, the hiprtc
// and HIP runtime versions, the target, the options (WOLOLO_JIT_FLAGS included), the embedded
// headers and the generated source; each part length-prefixed.
std::string jit_key(const char* src, const std::string& arch, bool count, const std::string& helper) {
    WoSha256 s;
    wo_sha256_init(&s);
    auto part = [&](const char* p, size_t n) {
        const uint64_t len = n;
        wo_sha256_update(&s, &len, sizeof len);
        wo_sha256_update(&s, p, n);
    };
    part("wololo-jit-2", 12);
    // the toolchain: hiprtc's major.minor and the HIP runtime's full version
    // (patch level included: a ROCm update that changes the compiler or the
    // device libraries misses instead of loading a stale object)
    // (queried once: hiprtcVersion waits while another thread's compile holds
    // hiprtc's lock, which stalled draw_frame behind a background compile)
    static const std::array<int, 3> ver = []() {
        int vmaj = 0, vmin = 0, vrt = 0;
        (void)hiprtcVersion(&vmaj, &vmin);
        (void)hipRuntimeGetVersion(&vrt);
        return std::array<int, 3>{vmaj, vmin, vrt};
    }();
    part((const char*)ver.data(), sizeof(int) * ver.size());
    // compiled by wo_jitc (the system hiprtc) rather than the hiprtc serving this process
    if (!helper.empty()) part("wo_jitc", 7);
    part(arch.data(), arch.size());
    for (const std::string& o : jit_options(arch, count)) part(o.data(), o.size());
    part(kEmbed_wo_device_common_h, strlen(kEmbed_wo_device_common_h));
    part(kEmbed_wo_scene_h, strlen(kEmbed_wo_scene_h));
    part(src, strlen(src));
    uint8_t dg[32];
    wo_sha256_final(&s, dg);
    char hex[65];
    wo_sha256_hex(dg, hex);
    return std::string(hex);
}

int jit_code(const char* src, const std::string& arch, bool count, JitCode* out, char* err, size_t errlen,
             const std::string& helper) {
    const auto t0 = std::chrono::steady_clock::now();
    for (const std::string& cc : compilers(helper)) {
        out->key = jit_key(src, arch, count, cc);
        out->origin = jit_lookup(out->key, &out->code);
        if (out->origin < 0) {
            if (jit_compile(cc, src, arch, count, out->code, err, errlen)) continue;
            out->origin = 2;
            (void)wo_jit_disk_store(out->key.c_str(), out->code.data(), out->code.size());  // best effort
            jit_cache_put(out->key, out->code);
        }
        out->seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        return 0;
    }
    return -1;  // `err` is the in-process compiler's, the last tried
}

// ELF64 little-endian, read with every offset checked against the n bytes before it is
// added to (a field may hold any value: the sums below cannot wrap).
bool kd_segment_sizes(const void* code, size_t n, const char* name, uint32_t* group, uint32_t* priv) {
    const unsigned char* b = static_cast<const unsigned char*>(code);
    auto rd = [&](uint64_t off, size_t len, uint64_t* v) {
        if (off > n || len > n - off) return false;
        uint64_t x = 0;
        for (size_t i = 0; i < len; ++i) x |= (uint64_t)b[off + i] << (8u * i);
        *v = x;
        return true;
    };
    if (n < 64 || memcmp(b, "\x7f" "ELF", 4) != 0 || b[4] != 2 || b[5] != 1) return false;
    uint64_t shoff, shentsize, shnum;
    if (!rd(0x28, 8, &shoff) || !rd(0x3a, 2, &shentsize) || !rd(0x3c, 2, &shnum) || shentsize < 64 || shoff > n)
        return false;
    // shoff <= n, i < 2^32 and shentsize < 2^16: no wrap
    auto sh = [&](uint64_t i, size_t field, size_t len, uint64_t* v) { return rd(shoff + i * shentsize + field, len, v); };
    const std::string want = std::string(name) + ".kd";
    const size_t want_n = want.size() + 1;  // with the terminator
    for (uint64_t i = 0; i < shnum; ++i) {
        uint64_t type, off, size, link, entsize;
        if (!sh(i, 4, 4, &type) || type != 2u) continue;  // SHT_SYMTAB
        if (!sh(i, 24, 8, &off) || !sh(i, 32, 8, &size) || !sh(i, 40, 4, &link) || !sh(i, 56, 8, &entsize) ||
            entsize < 24 || off > n || size > n - off)
            return false;
        uint64_t stroff, strsize;
        if (!sh(link, 24, 8, &stroff) || !sh(link, 32, 8, &strsize) || stroff > n || strsize > n - stroff) return false;
        for (uint64_t k = 0; entsize <= size - k; k += entsize) {  // k <= size <= n
            uint64_t nm, shndx, value;
            if (!rd(off + k, 4, &nm) || !rd(off + k + 6, 2, &shndx) || !rd(off + k + 8, 8, &value)) return false;
            if (nm >= strsize || want_n > strsize - nm) continue;
            if (memcmp(b + stroff + nm, want.c_str(), want_n) != 0) continue;
            uint64_t saddr, soff, g, p;
            if (!sh(shndx, 16, 8, &saddr) || !sh(shndx, 24, 8, &soff) || value < saddr || soff > n ||
                value - saddr > n - soff)
                return false;
            if (!rd(soff + (value - saddr), 4, &g) || !rd(soff + (value - saddr) + 4, 4, &p)) return false;
            *group = (uint32_t)g;
            *priv = (uint32_t)p;
            return true;
        }
    }
    return false;
}

}  // namespace wojit

using namespace wojit;

static std::string arch_or_default(const char* arch) { return arch ? arch : "gfx950"; }

extern "C" long long wo_jit_code_object(const char* src, const char* arch, int* origin, double* seconds,
                                        char* key_hex, char* err, size_t errlen) {
    JitCode jc;
    if (jit_code(src, arch_or_default(arch), false, &jc, err, errlen)) return -1;
    if (origin) *origin = jc.origin;
    if (seconds) *seconds = jc.seconds;
    if (key_hex) snprintf(key_hex, 65, "%s", jc.key.c_str());
    return (long long)jc.code.size();
}

extern "C" int wo_jit_code_resources(const char* src, const char* arch, uint32_t* out, char* err, size_t errlen) {
    JitCode jc;
    if (!src || !out) {
        snprintf(err, errlen, "no source");
        return -1;
    }
    if (jit_code(src, arch_or_default(arch), false, &jc, err, errlen)) return -1;
    uint32_t group = 0, priv = 0;
    if (!kd_segment_sizes(jc.code.data(), jc.code.size(), "wo_jit_pathtrace", &group, &priv)) {
        snprintf(err, errlen, "no kernel descriptor for wo_jit_pathtrace in the code object (%zu bytes)", jc.code.size());
        return -1;
    }
    out[0] = priv;
    out[1] = group;
    return 0;
}

extern "C" int wo_jit_compile_check(const char* src, const char* arch, char* err, size_t errlen) {
    std::vector<char> code;
    for (const std::string& cc : compilers(jitc_path()))
        if (jit_compile(cc, src, arch_or_default(arch), false, code, err, errlen) == 0) return 0;
    return -1;
}

// ---- background compiles (wo_dev.h WoJitJob) ----
struct WoJitJob {
    std::thread th;
    std::atomic<int> done{0};
    int rc = 0;
    std::string src, arch;
    char err[512] = {0};
};

WoJitJob* wojit::jit_job_start(const char* src, const std::string& arch) {
    WoJitJob* j = new (std::nothrow) WoJitJob();
    if (!j) return nullptr;
    j->src = src;
    j->arch = arch;
    try {
        j->th = std::thread([j]() {
            JitCode jc;
            j->rc = jit_code(j->src.c_str(), j->arch, false, &jc, j->err, sizeof j->err);
            j->done.store(1, std::memory_order_release);
        });
    } catch (...) {
        delete j;
        return nullptr;
    }
    return j;
}

extern "C" int wo_jit_job_done(WoJitJob* j) { return j->done.load(std::memory_order_acquire); }

extern "C" const char* wo_jit_job_source(WoJitJob* j) { return j->src.c_str(); }

extern "C" int wo_jit_job_finish(WoJitJob* j, char* err, size_t errlen) {
    if (j->th.joinable()) j->th.join();
    const int rc = j->rc;
    if (rc && err && errlen) snprintf(err, errlen, "%s", j->err);
    delete j;
    return rc;
}
