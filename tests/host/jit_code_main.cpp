// Stand-alone driver of the specialised kernels' code-object pipeline (csrc/jit_code.cpp):
//   jit_code_main <wo_jitc> <scratch cache directory> <generated source file>
// `make -C csgrenderer_amd/csrc jit-code-asan` builds it with -fsanitize=address,undefined
// and runs it; tests/test_jit_code.py runs the plain build.  Exits non-zero on the first
// failed expectation.  No GPU: hiprtc compiles for gfx950 anywhere.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <memory>

#include "jit_code.h"

using namespace wojit;

#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
            fprintf(stderr, __VA_ARGS__);                   \
            fprintf(stderr, " (%s)\n", #cond);              \
            exit(1);                                        \
        }                                                   \
    } while (0)

static const char kArch[] = "gfx950";
static const char kKernel[] = "wo_jit_pathtrace";

// the descriptor of the first `len` bytes of `code`, in an allocation of exactly `len`
// bytes with `width` bytes at `at` replaced by `value`'s low ones (width 0: unchanged)
static bool read_kd(const std::vector<char>& code, size_t len, size_t at, size_t width, uint64_t value, uint32_t* g,
                    uint32_t* p) {
    std::unique_ptr<char[]> copy(new char[len]);
    memcpy(copy.get(), code.data(), len);
    if (width) memcpy(copy.get() + at, &value, width);  // little-endian host, as the ELF
    return kd_segment_sizes(copy.get(), len, kKernel, g, p);
}

template <class T>
static T field(const std::vector<char>& code, size_t at) {  // of the unmutated, valid object
    T v;
    EXPECT(at <= code.size() && sizeof v <= code.size() - at, "field at %zu", at);
    memcpy(&v, code.data() + at, sizeof v);
    return v;
}

// A. the kernel-descriptor reader: the object, its prefixes, its fields set to hostile values
static void check_descriptor_reader(const std::vector<char>& code) {
    const size_t n = code.size();
    uint32_t group = 0, priv = ~0u;
    EXPECT(read_kd(code, n, 0, 0, 0, &group, &priv), "no descriptor in the object (%zu B)", n);
    EXPECT(priv == 0u && group > 0u, "group %u private %u", group, priv);
    for (size_t len = 0; len < n; ++len) {
        uint32_t g = 0, p = 0;
        if (read_kd(code, len, 0, 0, 0, &g, &p)) EXPECT(g == group && p == priv, "prefix %zu: %u %u", len, g, p);
    }
    const uint64_t values[] = {0ull, ~0ull, (uint64_t)n, (uint64_t)n - 1u, ~0ull - 9u, 1ull << 63};
    unsigned long reads = 0;
    auto mutate = [&](size_t at, size_t width) {
        for (uint64_t v : values) {
            uint32_t g, p;
            (void)read_kd(code, n, at, width, v, &g, &p);  // any answer: the sanitizer judges
            ++reads;
        }
    };
    mutate(0x28, 8);  // e_shoff, e_shentsize, e_shnum
    mutate(0x3a, 2);
    mutate(0x3c, 2);
    const uint64_t shoff = field<uint64_t>(code, 0x28);
    const size_t shentsize = field<uint16_t>(code, 0x3a), shnum = field<uint16_t>(code, 0x3c);
    size_t kd_sym = 0;
    for (size_t i = 0; i < shnum; ++i) {
        const size_t sh = shoff + i * shentsize;
        mutate(sh + 4, 4);   // sh_type
        mutate(sh + 16, 8);  // sh_addr
        mutate(sh + 24, 8);  // sh_offset
        mutate(sh + 32, 8);  // sh_size
        mutate(sh + 40, 4);  // sh_link
        mutate(sh + 56, 8);  // sh_entsize
        if (field<uint32_t>(code, sh + 4) != 2u) continue;  // SHT_SYMTAB: find `<kernel>.kd`
        const uint64_t off = field<uint64_t>(code, sh + 24), size = field<uint64_t>(code, sh + 32),
                       ent = field<uint64_t>(code, sh + 56);
        const uint64_t stroff = field<uint64_t>(code, shoff + field<uint32_t>(code, sh + 40) * shentsize + 24);
        for (uint64_t k = 0; k + ent <= size; k += ent)
            if (strcmp(code.data() + stroff + field<uint32_t>(code, off + k), (std::string(kKernel) + ".kd").c_str()) == 0)
                kd_sym = off + k;
    }
    EXPECT(kd_sym != 0, "no %s.kd symbol", kKernel);
    mutate(kd_sym, 4);      // st_name
    mutate(kd_sym + 6, 2);  // st_shndx
    mutate(kd_sym + 8, 8);  // st_value
    printf("descriptor reader: %zu B, group %u, private %u; %zu prefixes, %lu mutated reads\n", n, group, priv, n, reads);
}

// B. the process cache: 8 entries, least recently used first out
static void check_process_cache() {
    auto key = [](int i) { return "made-up-key-" + std::to_string(i); };
    std::vector<char> got;
    for (int i = 0; i < 9; ++i) jit_cache_put(key(i), std::vector<char>(16 + i, (char)i));
    EXPECT(!jit_cache_get(key(0), &got), "the first of 9 keys is still cached");
    for (int i = 1; i < 9; ++i)  // (got in put order: key 1 stays the oldest)
        EXPECT(jit_cache_get(key(i), &got) && got == std::vector<char>(16 + i, (char)i), "key %d", i);
    EXPECT(jit_cache_get(key(1), &got), "touch");
    jit_cache_put(key(9), std::vector<char>(1, 'x'));
    EXPECT(jit_cache_get(key(1), &got), "the touched key went");
    EXPECT(!jit_cache_get(key(2), &got), "the least recently used key stayed");
    EXPECT(jit_cache_get(key(9), &got) && got.size() == 1u, "the tenth key");
    printf("process cache: 8 entries, LRU\n");
}

// C. a helper that yields no object: the in-process compiler, under the in-process key
static std::vector<char> check_helper_fallback(const char* src, const std::string& jitc, const std::string& dir) {
    const std::string k_in = jit_key(src, kArch, false, ""), k_helper = jit_key(src, kArch, false, jitc);
    EXPECT(k_in != k_helper && k_in.size() == 64u, "keys %s %s", k_in.c_str(), k_helper.c_str());
    const std::string f_in = dir + "/" + k_in + ".co", f_helper = dir + "/" + k_helper + ".co";
    (void)unlink(f_in.c_str());  // an earlier run's
    (void)unlink(f_helper.c_str());
    char err[512] = "";
    JitCode broken, plain, real, again;
    EXPECT(jit_code(src, kArch, false, &broken, err, sizeof err, "/bin/false") == 0, "%s", err);
    EXPECT(broken.origin == 2 && broken.key == k_in, "origin %d key %s", broken.origin, broken.key.c_str());
    EXPECT(access(f_in.c_str(), R_OK) == 0 && access(f_helper.c_str(), F_OK) != 0, "cache files in %s", dir.c_str());
    EXPECT(jit_code(src, kArch, false, &plain, err, sizeof err, "") == 0, "%s", err);
    EXPECT(plain.key == broken.key && plain.code == broken.code, "helper \"\": key %s", plain.key.c_str());
    EXPECT(jit_code(src, kArch, false, &real, err, sizeof err, jitc) == 0, "%s", err);
    EXPECT(real.key == k_helper && real.origin == 2, "origin %d key %s", real.origin, real.key.c_str());
    EXPECT(access(f_helper.c_str(), R_OK) == 0, "%s", f_helper.c_str());
    EXPECT(jit_code(src, kArch, false, &again, err, sizeof err, jitc) == 0, "%s", err);
    EXPECT(again.origin == 0 && again.key == k_helper && again.code == real.code, "origin %d", again.origin);
    printf("helper fallback: in-process %.16s..., helper %.16s...\n", k_in.c_str(), k_helper.c_str());
    return broken.code;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: jit_code_main <wo_jitc> <cache directory> <source file>\n");
        return 2;
    }
    setenv("WOLOLO_JIT_CACHE", argv[2], 1);
    unsetenv("WOLOLO_JIT_FLAGS");
    std::string src;
    FILE* f = fopen(argv[3], "rb");
    EXPECT(f, "cannot read %s", argv[3]);
    char buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) src.append(buf, n);
    fclose(f);
    const std::vector<char> code = check_helper_fallback(src.c_str(), argv[1], argv[2]);
    check_descriptor_reader(code);
    check_process_cache();
    return 0;
}
