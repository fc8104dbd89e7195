// TEST-ONLY host instantiation of the item functions of the chain's own random numbers (hmcmt_items.h: item_philox4x32, item_rng_*,
// item_chain_draw_*).  Like emul_chain.cpp it is NOT part of the product: it holds the generator, the uniforms, the normals and the
// scalars against tests/rng_ref.py without a GPU, and the seeded momentum against item_chain_momentum fed with the same normals.
#include <cstdint>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

void emulrng_philox(const uint32_t* c, const uint32_t* k, uint32_t* out) { item_philox4x32(c, k, out); }

double emulrng_u52(uint32_t hi, uint32_t lo) { return item_rng_u52(hi, lo); }

void emulrng_normals(uint64_t seed, uint32_t stream, uint64_t t, int64_t a0, int64_t n, double* z) {
    for (int64_t i = 0; i < n; ++i) z[i] = item_rng_normal(seed, stream, t, (int)(a0 + i));
}

void emulrng_scalars(uint64_t seed, uint32_t stream, uint64_t t, int32_t Lmin, int32_t Lmax, int32_t* L, double* u) {
    int l = 0;
    item_rng_scalars(seed, stream, t, Lmin, Lmax, &l, u);
    *L = l;
}

// cell by cell what k_chain_draw_clip and k_chain_draw_momentum do, and k_chain_momentum on the clipped normals: zc[n], the two
// momenta p_draw[n] and p_fed[n], and each cell's term of p' M^-1 p from either route
void emulrng_momentum(uint64_t seed, uint32_t stream, uint64_t t, int64_t n, const double* invM, double* zc, double* p_draw, double* p_fed,
                      double* term_draw, double* term_fed) {
    for (int a = 0; a < (int)n; ++a) zc[a] = item_chain_draw_clip(seed, stream, t, a);
    for (int a = 0; a < (int)n; ++a) {
        term_draw[a] = item_chain_draw_momentum(seed, stream, t, invM, p_draw, a);
        term_fed[a] = item_chain_momentum(zc, invM, p_fed, a);
    }
}

}  // extern "C"
