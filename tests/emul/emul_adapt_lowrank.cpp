// TEST-ONLY host instantiation of the low-rank mass adaptation's item functions (hmcmt_items.h: item_adapt_lr_*, item_jacobi_eig),
// driven the way the kernels of kernels_chain.h (k_adapt_lr_mean, k_adapt_lr_gram, k_adapt_lr_lift, k_adapt_lr_sign) and
// chain_adapt_step / chain_adapt_lr_window_end (host_chain.h) drive them.  The window end's host maths is the product's own code:
// item_adapt_lr_estimate runs here exactly as it runs in the library.  NOT part of the product.
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../hmcmt2d_amd/csrc/hmcmt_items.h"

using namespace hmcmt;

extern "C" {

int emulalr_nmin() { return ADAPT_LR_NMIN; }
int emulalr_nmax() { return ADAPT_LR_NMAX; }
int emulalr_tile() { return ADAPT_LR_TILE; }
int emulalr_strip() { return ADAPT_LR_STRIP; }

// k_adapt_lr_mean: the two means and s = sqrt(invM)
void emulalr_mean(int32_t n, int64_t nAC, const double* X, const double* G, const double* invM, double* meanX, double* meanG, double* s) {
    for (int64_t a = 0; a < nAC; ++a) {
        meanX[a] = item_adapt_lr_mean(X, nAC, n, a);
        meanG[a] = item_adapt_lr_mean(G, nAC, n, a);
        s[a] = std::sqrt(invM[a]);
    }
}

// W [2n][nAC] as the kernels form it on the fly
void emulalr_w(int32_t n, int64_t nAC, const double* X, const double* G, const double* invM, double* W) {
    std::vector<double> mx((size_t)nAC), mg((size_t)nAC), s((size_t)nAC);
    emulalr_mean(n, nAC, X, G, invM, mx.data(), mg.data(), s.data());
    const double sq = std::sqrt((double)(n - 1));
    for (int i = 0; i < 2 * n; ++i)
        for (int64_t a = 0; a < nAC; ++a) W[(int64_t)i * nAC + a] = item_adapt_lr_w(X, G, mx.data(), mg.data(), s.data(), nAC, n, sq, i, a);
}

// k_adapt_lr_gram: the workgroups of the upper block triangle, thread (ti, tj) of tile (bi, bj) walking the cells strip by strip
void emulalr_gram(int32_t n, int64_t nAC, const double* X, const double* G, const double* invM, double* K) {
    const int N2 = 2 * n, T = (N2 + ADAPT_LR_TILE - 1) / ADAPT_LR_TILE;
    std::vector<double> W((size_t)N2 * nAC);
    emulalr_w(n, nAC, X, G, invM, W.data());
    for (int b = 0; b < T * (T + 1) / 2; ++b) {
        int t = b, bi = 0;
        while (t >= T - bi) { t -= T - bi; ++bi; }
        const int bj = bi + t;
        for (int ti = 0; ti < ADAPT_LR_TILE; ++ti)
            for (int tj = 0; tj < ADAPT_LR_TILE; ++tj) {
                const int i = bi * ADAPT_LR_TILE + ti, j = bj * ADAPT_LR_TILE + tj;
                if (i >= N2 || j >= N2) continue;
                double acc = 0.0;
                for (int64_t a0 = 0; a0 < nAC; a0 += ADAPT_LR_STRIP) {
                    const int64_t lim = nAC - a0 < ADAPT_LR_STRIP ? nAC - a0 : ADAPT_LR_STRIP;
                    for (int64_t c = 0; c < lim; ++c) acc = item_adapt_lr_dot(W[(size_t)i * nAC + a0 + c], W[(size_t)j * nAC + a0 + c], acc);
                }
                K[(int64_t)i * N2 + j] = acc;
                if (bi != bj) K[(int64_t)j * N2 + i] = acc;
            }
    }
}

// k_adapt_lr_lift through the per-output item function
void emulalr_lift(int32_t n, int64_t nAC, const double* X, const double* G, const double* invM, const double* B, int32_t r, double* U) {
    std::vector<double> mx((size_t)nAC), mg((size_t)nAC), s((size_t)nAC);
    emulalr_mean(n, nAC, X, G, invM, mx.data(), mg.data(), s.data());
    const double sq = std::sqrt((double)(n - 1));
    for (int k = 0; k < r; ++k)
        for (int64_t a = 0; a < nAC; ++a) U[(int64_t)k * nAC + a] = item_adapt_lr_lift(X, G, mx.data(), mg.data(), s.data(), B, nAC, n, sq, r, k, a);
}

// k_adapt_lr_sign: 256 threads scan their cells, the tree of the workgroup, the flip
void emulalr_sign(int64_t nAC, int32_t r, double* U) {
    for (int k = 0; k < r; ++k) {
        double* u = U + (int64_t)k * nAC;
        double shV[256];
        long long shA[256];
        for (int t = 0; t < 256; ++t) {
            double best = -1.0;
            long long at = nAC;
            for (int64_t a = t; a < nAC; a += 256) {
                const double v = std::fabs(u[a]);
                if (item_adapt_lr_beats(v, a, best, at)) { best = v; at = a; }
            }
            shV[t] = best; shA[t] = at;
        }
        for (int o = 128; o > 0; o >>= 1)
            for (int t = 0; t < o; ++t)
                if (item_adapt_lr_beats(shV[t + o], shA[t + o], shV[t], shA[t])) { shV[t] = shV[t + o]; shA[t] = shA[t + o]; }
        if (shA[0] >= nAC || !(u[shA[0]] < 0.0)) continue;
        for (int64_t a = 0; a < nAC; ++a) u[a] = -u[a];
    }
}

// item_jacobi_eig: A [n][n] symmetric (kept), d ascending, Vt[k][.] the eigenvector of d[k]; returns the sweeps
int emulalr_jacobi(int32_t n, const double* A, double* Vt, double* d) {
    std::vector<double> a(A, A + (size_t)n * n);
    return item_jacobi_eig(n, a.data(), Vt, d);
}

// item_adapt_lr_estimate: out[0..3] = m, r, fallback; thetaAll [2n], theta [rank], B [2n][rank] row-major with r columns used.
// geometric == 0 is the exact-answer test's counter-example and NOT the product's: between the product's projection and its selection
// the arithmetic mean (Cd + Cg^-1) / 2 stands in Sigma's place.
void emulalr_estimate(int32_t n, const double* K, int32_t rank, double cutoff, double gamma, int32_t geometric, int32_t* out, double* thetaAll,
                      double* theta, double* B) {
    AdaptLrEstimate E;
    E.fallback = 1;
    if (geometric) {
        E = item_adapt_lr_estimate(n, K, rank, cutoff, gamma);
    } else {
        std::vector<double> T, Cd, Cg;
        const int m = item_adapt_lr_project(n, K, gamma, T, Cd, Cg);
        if (m > 0) {
            std::vector<double> A(Cg), Vt((size_t)m * m), d((size_t)m), Sig((size_t)m * m), Yt((size_t)m * m), th((size_t)m);
            item_jacobi_eig(m, A.data(), Vt.data(), d.data());
            for (int i = 0; i < m; ++i)
                for (int j = 0; j < m; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < m; ++k) acc += Vt[(size_t)k * m + i] / d[k] * Vt[(size_t)k * m + j];
                    Sig[(size_t)i * m + j] = 0.5 * (Cd[(size_t)i * m + j] + acc);
                }
            item_adapt_lr_symmetrise(m, Sig);
            item_jacobi_eig(m, Sig.data(), Yt.data(), th.data());
            E = item_adapt_lr_select(n, m, T, Yt, th, rank, cutoff);
        }
    }
    out[0] = E.m; out[1] = E.r; out[2] = E.fallback;
    for (size_t i = 0; i < E.thetaAll.size(); ++i) thetaAll[i] = E.thetaAll[i];
    for (size_t i = 0; i < E.theta.size(); ++i) theta[i] = E.theta[i];
    for (size_t i = 0; i < E.B.size(); ++i) B[i] = E.B[i];
}

// chain_adapt_step's bookkeeping of the stores over a whole warm-up: slot[c] = the row step c is stored in (-1: not stored);
// per closed window (at most 64) end[w] = its last step, stored[w], stride[w].  Returns the windows closed.
int emulalr_schedule(int64_t nwarmup, int32_t initBuffer, int32_t termBuffer, int32_t baseWindow, int32_t maxSamples, int32_t* slot,
                     int64_t* end, int32_t* storedOut, int64_t* strideOut) {
    long long wsize = baseWindow, wnext = (long long)initBuffer + baseWindow - 1, wcount = 0;
    long long winStart = initBuffer, stride = item_adapt_lr_stride(wnext - initBuffer + 1, maxSamples);
    int stored = 0, nw = 0;
    for (long long c = 0; c < nwarmup; ++c) {
        slot[c] = -1;
        const bool inWindow = c >= initBuffer && c < nwarmup - termBuffer;
        if (inWindow) {
            ++wcount;
            const long long i = c - winStart;
            if (i >= 0 && item_adapt_lr_due(i, stride) && stored < maxSamples) slot[c] = stored++;
        }
        if (inWindow && c == wnext) {
            if (wcount >= 2 && nw < 64) { end[nw] = c; storedOut[nw] = stored; strideOut[nw] = stride; ++nw; }
            wcount = 0;
            wnext = item_adapt_next_window(c, &wsize, nwarmup, termBuffer);
            winStart = c + 1;
            stride = wnext >= 0 ? item_adapt_lr_stride(wnext - c, maxSamples) : 1;
            stored = 0;
        }
    }
    return nw;
}

}  // extern "C"
