// Stand-alone driver of the lane BVH builder (csrc/lane_bvh_build.cpp) for sanitizer
// runs: `make -C csgrenderer_amd/csrc lane-bvh-asan DUMPS="..."` compiles both with
// -fsanitize=address,undefined and runs the builder over scene dumps
// (dump_scenes.py: u32 n_recs, n_prims, n_mats; the records; the materials).
#include <stdio.h>

#include <vector>

#include "wo_dev.h"

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        FILE* f = fopen(argv[i], "rb");
        uint32_t n[3];
        if (!f || fread(n, sizeof n[0], 3, f) != 3) {
            fprintf(stderr, "%s: cannot read\n", argv[i]);
            return 1;
        }
        // exact sizes, so that a read past either table is the sanitizer's
        std::vector<WoRec> prog(n[0]);
        std::vector<WoMaterial> mats(n[2]);
        if (fread(prog.data(), sizeof(WoRec), n[0], f) != n[0] || fread(mats.data(), sizeof(WoMaterial), n[2], f) != n[2]) {
            fprintf(stderr, "%s: truncated\n", argv[i]);
            return 1;
        }
        fclose(f);
        wolbvh::LaneBvhBuild b;
        char err[256] = "";
        if (wolbvh::lane_bvh_build(prog.data(), n[0], n[1], mats.data(), n[2], &b, err, sizeof err)) {
            fprintf(stderr, "%s: %s\n", argv[i], err);
            return 1;
        }
        const WoLaneBvhDesc& d = b.desc;
        printf("%s: %u nodes, depth %u, top %u, always %u, terms %u, wide %u, general %u, blob %zu B, LDS %zu B\n", argv[i],
               d.nodes, d.depth, d.top, d.always, d.terms, d.wide, d.general, b.blob.size(), wolbvh::lane_bvh_lds(d));
    }
    return 0;
}
