// codec_plan_main.cpp — prints what csrc/codec_plan.h plans for every conv weight of a DAC decoder; tests/test_codec_plan_cpu.py builds it with
// the host compiler (no HIP), runs it and holds the expected tables.
//   codec_plan_main LATENT C0 STRIDE[,STRIDE...] [knob=value ...]      knobs: the fields of CodecKnobs
// One line per layer: name kind scheme co_t ci_t ns kt transposed elems.  The three units of a block have the same dims: one k7 / k1 line per block.
#include "../tts.cpp_amd/csrc/codec_plan.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

static const char *KIND[] = {"none", "f32_tile", "f32_direct", "f16_tile", "b3", "planes", "unit_pair", "unit_tap", "convt_planes"};

static void row(const std::string &name, const CodecImage &p) {
    if (p.w != nullptr) { fprintf(stderr, "%s: a plan carries no device pointer\n", name.c_str()); exit(2); }
    printf("%s %s %d %d %d %d %d %d %zu\n", name.c_str(), KIND[p.kind], (int) p.scheme, p.co_t, p.ci_t, p.ns, p.kt, (int) p.transposed, p.elems);
}

int main(int argc, char **argv) {
    if (argc < 4) { fprintf(stderr, "usage: %s LATENT C0 STRIDES [knob=value ...]\n", argv[0]); return 2; }
    const int latent = atoi(argv[1]), c0 = atoi(argv[2]);
    std::vector<int> strides;
    for (char *t = strtok(argv[3], ","); t; t = strtok(nullptr, ",")) strides.push_back(atoi(t));
    CodecKnobs k;
    struct { const char *name; int *field; } fields[] = {
        {"valu", &k.valu}, {"f16", &k.f16}, {"b3", &k.b3}, {"fuse", &k.fuse}, {"planes", &k.planes}, {"split", &k.split}, {"f16_planes", &k.f16_planes},
        {"tap7", &k.tap7}, {"convt_b3", &k.convt_b3}, {"conv1_direct", &k.conv1_direct}, {"kk_split", &k.kk_split}, {"kk_b3", &k.kk_b3}, {"kk_mfma", &k.kk_mfma}};
    for (int i = 4; i < argc; i++) {
        const char *eq = strchr(argv[i], '=');
        bool found = false;
        for (auto &f : fields)
            if (eq && strlen(f.name) == (size_t) (eq - argv[i]) && !strncmp(f.name, argv[i], eq - argv[i])) { *f.field = atoi(eq + 1); found = true; }
        if (!found) { fprintf(stderr, "unknown knob '%s'\n", argv[i]); return 2; }
    }
    row("init", codec_plan(ROLE_INIT, c0, latent, 7, 1, k));
    int C = c0;
    for (size_t i = 0; i < strides.size(); i++) {
        const std::string b = "b" + std::to_string(i);
        row(b + ".convt", codec_plan(ROLE_CONVT, C / 2, C, 2 * strides[i], strides[i], k));
        C /= 2;
        row(b + ".k7", codec_plan(ROLE_UNIT7, C, C, 7, 1, k));
        row(b + ".k1", codec_plan(ROLE_UNIT1, C, C, 1, 1, k));
    }
    return 0;
}
