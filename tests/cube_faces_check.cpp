// cube_faces_check -- rend3_amd/csrc/cube_faces.h compiled alone (no HIP, no context), built with the address and
// undefined-behaviour sanitizers and run as a child process by tests/test_skybox_lod.py.
//
// usage: cube_faces_check TABLE.  TABLE is written by the test from tests/skybox_reference.py resolve_texel: per extent a line
// "n <n>" followed by 6 * (n + 2)^2 integers, row-major per bordered face: the id face * n * n + j * n + i of the texel the
// position holds, or -1 for a corner.  Every face is assembled over exactly sized host arrays, once with one-word texels and once
// with 16-byte texels, and compared with the table.  Prints one line per extent and the pool layout of some chains; FAIL lines
// name what differs.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../rend3_amd/csrc/cube_faces.h"

struct Texel16 {
    uint32_t w[4];
};

static int check_extent(uint32_t n, const std::vector<long> &want) {
    const size_t dense_texels = (size_t)n * n, face_texels = (size_t)(n + 2u) * (n + 2u);
    int bad = 0;
    // one word per texel: texel id + 1 (0 is the corner's zero)
    std::vector<uint32_t> dense(6u * dense_texels);
    for (size_t k = 0; k < dense.size(); ++k) dense[k] = (uint32_t)k + 1u;
    std::vector<Texel16> dense16(6u * dense_texels);
    for (size_t k = 0; k < dense16.size(); ++k) dense16[k] = Texel16{{(uint32_t)k + 1u, 7u, (uint32_t)k ^ 0x55u, n}};
    for (uint32_t f = 0; f < 6u; ++f) {
        std::vector<uint32_t> out(face_texels, 0xDEADBEEFu);
        std::vector<Texel16> out16(face_texels, Texel16{{9u, 9u, 9u, 9u}});
        for (uint32_t u = 0; u < face_texels; ++u) {
            cube_faces::assemble_at(dense.data(), dense_texels, out.data(), f, n, u, 0u);
            cube_faces::assemble_at(dense16.data(), dense_texels, out16.data(), f, n, u, Texel16{{0u, 0u, 0u, 0u}});
        }
        for (uint32_t u = 0; u < face_texels; ++u) {
            const long w = want[(size_t)f * face_texels + u];
            const uint32_t expect = w < 0 ? 0u : (uint32_t)w + 1u;
            const Texel16 e16 = w < 0 ? Texel16{{0u, 0u, 0u, 0u}} : dense16[(size_t)w];
            const Texel16 &g = out16[u];
            if (out[u] != expect || g.w[0] != e16.w[0] || g.w[1] != e16.w[1] || g.w[2] != e16.w[2] || g.w[3] != e16.w[3]) {
                if (bad < 8) std::printf("FAIL n %u face %u position %u: got %u, want %u\n", n, f, u, out[u], expect);
                ++bad;
            }
        }
    }
    return bad;
}

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::FILE *fp = std::fopen(argv[1], "r");
    if (!fp) return 2;
    unsigned n = 0;
    int bad = 0;
    while (std::fscanf(fp, " n %u", &n) == 1) {
        std::vector<long> want(6u * (size_t)(n + 2u) * (n + 2u));
        for (long &w : want)
            if (std::fscanf(fp, "%ld", &w) != 1) return 2;
        const int b = check_extent(n, want);
        std::printf("extent_%u %d\n", n, b);
        bad += b;
    }
    std::fclose(fp);
    // the pool layout: (N, mips, per_texel) -> level starts and the cube's words
    const uint32_t chains[][3] = {{1, 1, 1}, {1, 1, 4}, {3, 2, 1}, {5, 3, 4}, {8, 4, 1}, {64, 7, 4}, {16384, 15, 1}};
    for (const auto &c : chains) {
        std::printf("layout_%u_%u_%u", c[0], c[1], c[2]);
        for (uint32_t k = 0; k <= c[1]; ++k) std::printf(" %llu", (unsigned long long)cube_faces::level_start(c[0], k, c[2]));
        std::printf("\n");
    }
    return bad ? 1 : 0;
}
