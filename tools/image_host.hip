// Host build of image.hip's per-pixel arithmetic (mipsfusion_amd/csrc/image_dev.h), for checking it without a GPU
// (tests/test_image_cpu.py):
//     image_host <in> <out>
// <in>:  uint32 n, H, W, C, dtype (0 fp32, 1 fp64), reserved; double window[11], C1, C2; a[n*H*W*C]; b[n*H*W*C].
// <out>: error records [n] (32 bytes each); the pool of a, double [n,Ho,Wo,C]; and, when H and W are at least 11, the ssim map and
//        the cs map, double [n,C,H-10,W-10] each, and the ssim records [n*C] (32 bytes each).
// The loops follow the kernels: every tile of every (view, channel) staged with its halo, the first pass into five planes, the
// second at the two positions of each of the 256 threads, and the sums lane by lane: butterfly, waves ascending, partials, one
// finishing wave.  Nothing here launches a kernel.  This is also the program to build with -Xarch_host -fsanitize=address,undefined.
#include "../mipsfusion_amd/csrc/image_dev.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace mipsf::image;

namespace {

constexpr int TPB = 256, WAVE = 64, WAVES = TPB / WAVE;

struct AddOp {
    double operator()(double x, double y) const { return x + y; }
};
struct MaxOp {
    double operator()(double x, double y) const { return max_keep(x, y); }
};

// what lane 0 of a wave holds after the butterfly
template <class Op>
double butterfly(const double* lanes, Op op) {
    double v[WAVE], t[WAVE];
    for (int l = 0; l < WAVE; ++l) v[l] = lanes[l];
    for (int o = 32; o > 0; o >>= 1) {
        for (int l = 0; l < WAVE; ++l) t[l] = op(v[l], v[l ^ o]);
        for (int l = 0; l < WAVE; ++l) v[l] = t[l];
    }
    return v[0];
}
template <class Op>
double block_reduce(const double* threads, Op op) {
    double r = butterfly(threads, op);
    for (int w = 1; w < WAVES; ++w) r = op(r, butterfly(threads + w * WAVE, op));
    return r;
}
// one finishing wave over m partials with a stride between them
template <class Op>
double finish(const double* p, size_t m, size_t stride, Op op) {
    double lanes[WAVE];
    for (int l = 0; l < WAVE; ++l) {
        double s = 0.0;
        for (size_t k = l; k < m; k += WAVE) s = op(s, p[k * stride]);
        lanes[l] = s;
    }
    return butterfly(lanes, op);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 1;
    FILE* in = fopen(argv[1], "rb");
    uint32_t h[6];
    double k[13];
    if (!in || fread(h, 4, 6, in) != 6 || fread(k, 8, 13, in) != 13) return 2;
    const uint32_t n = h[0], H = h[1], W = h[2], C = h[3], dtype = h[4];
    if (!n || !H || !W || !C || C > MIPSF_IMAGE_MAX_CHANNELS || dtype > 1) return 2;
    const size_t m = (size_t)H * W * C, total = m * n;
    std::vector<double> a(total), b(total);
    for (std::vector<double>* dst : {&a, &b}) {
        if (dtype == MIPSF_IMAGE_F32) {
            std::vector<float> raw(total);
            if (fread(raw.data(), 4, total, in) != total) return 3;
            for (size_t i = 0; i < total; ++i) (*dst)[i] = (double)raw[i];
        } else if (fread(dst->data(), 8, total, in) != total) {
            return 3;
        }
    }
    fclose(in);
    Window win;
    for (int t = 0; t < TAPS; ++t) win.w[t] = k[t];
    const double C1 = k[11], C2 = k[12];
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 4;

    // ---- mipsf_image_error
    const uint32_t nb = (uint32_t)std::min<size_t>((m + TPB - 1) / TPB, MIPSF_IMAGE_ERROR_MAX_BLOCKS);
    for (uint32_t v = 0; v < n; ++v) {
        std::vector<double> part((size_t)nb * 3);
        for (uint32_t blk = 0; blk < nb; ++blk) {
            double sq[TPB], ab[TPB], mx[TPB];
            for (int t = 0; t < TPB; ++t) {
                sq[t] = ab[t] = mx[t] = 0.0;
                for (size_t p = (size_t)blk * TPB + t; p < m; p += (size_t)nb * TPB) {
                    const double d = a[v * m + p] - b[v * m + p];
                    const double dd = d * d, da = std::fabs(d);
                    sq[t] = sq[t] + dd;
                    ab[t] = ab[t] + da;
                    mx[t] = max_keep(mx[t], da);
                }
            }
            part[blk * 3 + 0] = block_reduce(sq, AddOp()), part[blk * 3 + 1] = block_reduce(ab, AddOp()), part[blk * 3 + 2] = block_reduce(mx, MaxOp());
        }
        mipsf_image_error_record rec = {finish(part.data(), nb, 3, AddOp()), finish(part.data() + 1, nb, 3, AddOp()),
                                        finish(part.data() + 2, nb, 3, MaxOp()), (uint64_t)m};
        if (fwrite(&rec, sizeof rec, 1, out) != 1) return 5;
    }

    // ---- mipsf_image_pool2 of a
    {
        const uint32_t Ho = pool_out(H), Wo = pool_out(W);
        std::vector<double> pooled((size_t)n * Ho * Wo * C);
        for (size_t e = 0; e < pooled.size(); ++e) {
            const uint32_t ch = (uint32_t)(e % C), j = (uint32_t)(e / C % Wo), i = (uint32_t)(e / C / Wo % Ho), view = (uint32_t)(e / C / Wo / Ho);
            const double* img = a.data() + (size_t)view * m + ch;
            pooled[e] = pool_pixel(H, W, i, j, [&](uint32_t r, uint32_t c) { return img[((size_t)r * W + c) * C]; });
        }
        if (fwrite(pooled.data(), 8, pooled.size(), out) != pooled.size()) return 5;
    }

    // ---- mipsf_image_ssim
    if (H >= MIPSF_IMAGE_WINDOW && W >= MIPSF_IMAGE_WINDOW) {
        const uint32_t Ho = H - HALO, Wo = W - HALO, ntx = tiles_x(W), nty = tiles_y(H), tiles = ntx * nty;
        std::vector<double> map_ssim((size_t)n * C * Ho * Wo), map_cs(map_ssim.size());
        std::vector<mipsf_image_ssim_record> recs((size_t)n * C);
        static double X[IN_H][IN_W], Y[IN_H][IN_W], G[5][TILE_H][IN_W];
        for (uint32_t plane = 0; plane < n * C; ++plane) {
            const uint32_t view = plane / C, ch = plane % C;
            const size_t base = (size_t)view * m + ch;
            std::vector<double> part((size_t)tiles * 2);
            for (uint32_t tile = 0; tile < tiles; ++tile) {
                const uint32_t r0 = tile / ntx * TILE_H, c0 = tile % ntx * TILE_W;
                for (int r = 0; r < IN_H; ++r)
                    for (int c = 0; c < IN_W; ++c) {
                        const bool inside = r0 + r < H && c0 + c < W;
                        const size_t off = inside ? base + ((size_t)(r0 + r) * W + (c0 + c)) * C : base;
                        X[r][c] = inside ? a[off] : 0.0;
                        Y[r][c] = inside ? b[off] : 0.0;
                    }
                for (int r = 0; r < TILE_H; ++r)
                    for (int c = 0; c < IN_W; ++c) {
                        double g[5];
                        pass_h(win, &X[r][c], &Y[r][c], IN_W, g);
                        for (int q = 0; q < 5; ++q) G[q][r][c] = g[q];
                    }
                double ts[TPB], tc[TPB];
                for (int t = 0; t < TPB; ++t) {
                    double vs[2], vc[2];
                    for (int hh = 0; hh < 2; ++hh) {
                        const int r = t / TILE_W + hh * (TILE_H / 2), c = t % TILE_W;
                        double f[5], s, cs;
                        for (int q = 0; q < 5; ++q) f[q] = filter11(win, &G[q][r][c], 1);
                        ssim_cs(f, C1, C2, s, cs);
                        const bool valid = r0 + r < Ho && c0 + c < Wo;
                        vs[hh] = valid ? s : 0.0, vc[hh] = valid ? cs : 0.0;
                        if (valid) {
                            const size_t o = ((size_t)plane * Ho + (r0 + r)) * Wo + (c0 + c);
                            map_ssim[o] = s, map_cs[o] = cs;
                        }
                    }
                    ts[t] = vs[0] + vs[1], tc[t] = vc[0] + vc[1];
                }
                part[tile * 2 + 0] = block_reduce(ts, AddOp()), part[tile * 2 + 1] = block_reduce(tc, AddOp());
            }
            recs[plane] = mipsf_image_ssim_record{finish(part.data(), tiles, 2, AddOp()), finish(part.data() + 1, tiles, 2, AddOp()),
                                                  (uint64_t)Ho * Wo, 0};
        }
        if (fwrite(map_ssim.data(), 8, map_ssim.size(), out) != map_ssim.size() || fwrite(map_cs.data(), 8, map_cs.size(), out) != map_cs.size() ||
            fwrite(recs.data(), sizeof(mipsf_image_ssim_record), recs.size(), out) != recs.size())
            return 5;
    }
    fclose(out);
    printf("%u views of %u x %u x %u\n", n, H, W, C);
    return 0;
}
