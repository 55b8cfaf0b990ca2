// Host build of raster.hip's screen box and pixel test, for checking them without a GPU (tests/test_raster_cpu.py):
//     raster_host <in> <out>
// <in>: uint32 V, F, n, H, W; double fx, fy, cx, cy, near, far; float vertices[V*3]; int32 faces[F*3]; float poses[n*16].
// <out>: uint64 keys[n*H*W], what mipsf_raster_depth's key buffer holds before the resolve.  The loops follow the kernels: every
// (view, face) pair's tile box from face_setup, every tile of it by its number, 64 lanes a tile, the smallest key kept.
#include "../mipsfusion_amd/csrc/raster.hip"

#include <cstdio>
#include <vector>

namespace mipsf {       // what capi.hip gives the library; nothing here launches a kernel
void set_error(const char*, ...) {}
int check_launch(const char*) { return 0; }
int device_cus() { return 0; }
}  // namespace mipsf

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = fopen(argv[1], "rb");
    uint32_t h[5];
    double k[6];
    if (!in || fread(h, 4, 5, in) != 5 || fread(k, 8, 6, in) != 6) return 2;
    const uint32_t V = h[0], F = h[1], n = h[2], H = h[3], W = h[4];
    std::vector<float> v((size_t)V * 3), p((size_t)n * 16);
    std::vector<int32_t> f((size_t)F * 3);
    if (fread(v.data(), 4, v.size(), in) != v.size() || fread(f.data(), 4, f.size(), in) != f.size() ||
        fread(p.data(), 4, p.size(), in) != p.size())
        return 3;
    fclose(in);
    const Scene s = {v.data(), f.data(), p.data(), V, F, n, H, W, k[0], k[1], k[2], k[3], k[4], k[5]};
    std::vector<uint64_t> keys((size_t)n * H * W, KEY_EMPTY);
    unsigned long long tiles = 0, whole = 0;
    for (uint32_t item = 0; item < n * F; ++item) {
        const uint32_t view = item / F, face = item % F;
        Face o;
        const TileBox b = face_setup(s, view, face, o);
        const uint64_t count = (uint64_t)b.nx * b.ny;
        if (b.nx && (b.x0 + b.nx > (W + TILE - 1) / TILE || b.y0 + b.ny > (H + TILE - 1) / TILE)) return 4;      // a box outside the image
        tiles += count, whole += count == (uint64_t)((W + TILE - 1) / TILE) * ((H + TILE - 1) / TILE);
        for (uint64_t local = 0; local < count; ++local)
            for (uint32_t lane = 0; lane < MIPSF_WAVE; ++lane) {
                const uint32_t i = (b.x0 + (uint32_t)(local % b.nx)) * TILE + (lane & 7u);
                const uint32_t j = (b.y0 + (uint32_t)(local / b.nx)) * TILE + (lane >> 3);
                uint64_t key;
                if (i < W && j < H && pixel_key(s, o, face, i, j, key)) {
                    uint64_t& q = keys[((size_t)view * H + j) * W + i];
                    if (key < q) q = key;
                }
            }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out || fwrite(keys.data(), 8, keys.size(), out) != keys.size()) return 5;
    fclose(out);
    printf("%u pairs, %llu tiles, %llu pairs with the whole image\n", n * F, tiles, whole);
    return 0;
}
