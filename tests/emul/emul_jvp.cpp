// TEST-ONLY host instantiation of the matrix-free Jacobian products (hmcmt_items.h: item_dsigma .. item_tangent_data,
// item_vbar_free, jtvp_cell) on top of the emulation's serial driver and its own COCG solver (emul.cpp, included as it is).
// Like emul.cpp it is NOT part of the product: it exists so that the tangent-linear arithmetic and the free-u adjoint can be held
// against the oracle without a GPU.
#include "emul.cpp"

namespace {

struct EmulJvp {
    Emul e;
    std::vector<double> dSig, gPart2;
    std::vector<cplx> dBC, dbcL, dbcR, dbcB, dF, jv, u;
    std::vector<double> tanV;
    bool linearized = false;

    void bind() {
        e.bind();
        const HostProblem& h = e.hp;
        View& v = e.v;
        // (emul.cpp's driver predates the tipper: the functional count, the per-functional arrays and the tipper's tables)
        v.nTip = h.nTip;
        if (h.nTip) {
            v.nRx = h.nFun;
            e.Zrx.assign((size_t)h.S * h.nFun, cplx{0, 0}); e.rxN0.assign((size_t)h.S * h.nFun, 0);
            e.rxD.assign((size_t)h.S * h.nFun * 11, cplx{0, 0}); e.rxCoef.assign((size_t)h.S * h.nFun, cplx{0, 0});
            v.Zrx = e.Zrx.data(); v.rxN0 = e.rxN0.data(); v.rxD = e.rxD.data(); v.rxCoef = e.rxCoef.data();
            v.rxCL = h.rxCL.data(); v.rxCR = h.rxCR.data(); v.rxVL = h.rxVL.data(); v.rxVR = h.rxVR.data();
        }
        dSig.assign(h.nCell, 0); tanV.assign(h.nAC, 0);
        dBC.assign((size_t)h.S * 2 * h.nz * h.nz, cplx{0, 0});
        dbcL.assign((size_t)h.S * h.nz, cplx{0, 0}); dbcR = dbcL; dbcB.assign((size_t)h.S * (h.ny + 1), cplx{0, 0});
        dF.assign((size_t)h.S * v.vstride, cplx{0, 0});
        jv.assign(h.nData, cplx{0, 0}); u = jv;
        v.dBC = dBC.data(); v.dSig = dSig.data(); v.tanV = tanV.data();
        v.dbcL = dbcL.data(); v.dbcR = dbcR.data(); v.dbcB = dbcB.data(); v.dF = dF.data(); v.jv = jv.data(); v.uData = u.data();
    }

    // hmcmt_linearize: the forward evaluation with the receiver derivatives, then the boundary-sensitivity tables
    void linearize(const double* m, int kind, double tol, int maxit) {
        double mis = 0;
        const View& V = e.v;
        // (run(wantGrad = false) stops behind the misfit: forward fields, Zrx; the derivatives of the functionals come next)
        e.run(m, false, kind, tol, maxit, &mis);
        for (int s = 0; s < V.S; ++s) for (int r = 0; r < V.nRx; ++r) item_rx(V, s, r, true);
        for (int s = 0; s < V.S; ++s) for (int prof = 0; prof < 3; ++prof) {
            for (int j = 0; j <= V.nz; ++j) item_sens_layers(V, s, prof, j);
            item_sens_profile(V, s, prof);
            for (int c = 0; c < V.nz; ++c) item_bcsens_pre(V, s, prof, c);
        }
        linearized = true;
    }

    int jvp(const double* vin, int wrt, int kind, double tol, int maxit, double* out) {
        if (!linearized) return -1;
        const View& V = e.v;
        std::memcpy(tanV.data(), vin, sizeof(double) * V.nAC);
        for (int c = 0; c < V.nCell; ++c) item_dsigma(V, c, wrt);
        for (int s = 0; s < V.S; ++s) {
            for (int prof = 0; prof < 2; ++prof) for (int iz = 1; iz <= V.nz; ++iz) item_dbc_side(V, s, prof, iz);
            for (int iy = 1; iy <= V.ny - 1; ++iy) item_dbc_bottom(V, s, iy);
        }
        for (int s = 0; s < V.S; ++s)
            for (int iz = 0; iz < V.NZP; ++iz) for (int iy = 0; iy < V.NYP; ++iy) item_tangent_rhs(V, s, iy, iz);
        std::fill(dF.begin(), dF.end(), cplx{0, 0});
        for (int s = 0; s < V.S; ++s) if (V.sysOn[s]) e.cocg(s, dF.data() + (long)s * V.vstride, kind, tol, maxit);
        std::fill(jv.begin(), jv.end(), cplx{0, 0});
        for (int s = 0; s < V.S; ++s) for (int r = 0; r < V.nRx; ++r) item_tangent_data(V, s, r);
        std::memcpy(out, jv.data(), sizeof(cplx) * V.nData);
        return 0;
    }

    int jtvp(const double* uin, int wrt, int kind, double tol, int maxit, double* out) {
        if (!linearized) return -1;
        const View& V = e.v;
        std::memcpy(u.data(), uin, sizeof(cplx) * V.nData);
        for (int p = 0; p < V.nData; ++p) item_vbar_free(V, p);
        for (int s = 0; s < V.S; ++s) for (int r = 0; r < V.nRx; ++r) item_rxcoef(V, s, r);
        std::fill(e.R.begin(), e.R.end(), cplx{0, 0});
        std::fill(e.srcB.begin(), e.srcB.end(), cplx{0, 0});
        for (int s = 0; s < V.S; ++s) for (int row = 0; row < 2; ++row) for (int iy = 0; iy <= V.ny; ++iy) item_src(V, s, row, iy);
        std::fill(e.Lam.begin(), e.Lam.end(), cplx{0, 0});
        for (int s = 0; s < V.S; ++s) if (V.sysOn[s]) e.cocg(s, e.Lam.data() + (long)s * V.vstride, kind, tol, maxit);
        for (int s = 0; s < V.S; ++s) {
            for (int iz = 1; iz <= V.nz; ++iz) item_wside(V, s, iz);
            for (int ky = 0; ky < V.ny; ++ky) item_colw(V, s, ky);
            for (int prof = 0; prof < 2; ++prof) for (int c = 0; c < V.nz; ++c) item_bcsens_contract(V, s, prof, c);
        }
        for (int mode = 0; mode < 2; ++mode) for (int c = 0; c < V.nCell; ++c) item_gradcell(V, mode, c);
        for (int s = 0; s < V.S; ++s) for (int ky = 0; ky < V.ny; ++ky) item_qterm(V, s, ky);
        for (int a = 0; a < V.nAC; ++a) out[a] = jtvp_cell(V, a, wrt, V.gPart, 2);
        return 0;
    }
};

}  // namespace

extern "C" {

void* emuljvp_create(int64_t ny, int64_t nz, const double* yLen, const double* zLen, const double* origin,
                     int64_t nFreq, const double* freqs, int64_t nRx, const double* rxY, const double* rxZ,
                     int64_t nComp, const int64_t* compMode, int64_t nData, const int64_t* freqID,
                     const int64_t* rxID, const int64_t* dtID, const uint8_t* dataID, const double* obs,
                     const double* dataW, int64_t nAC, const int64_t* activeIdx, const double* bgModel,
                     char* err, int errlen) {
    EmulJvp* j = new EmulJvp();
    if (!j->e.hp.build(ny, nz, yLen, zLen, origin, nFreq, freqs, nRx, rxY, rxZ, nComp, compMode, nData, freqID,
                       rxID, dtID, dataID, obs, dataW, nAC, activeIdx, bgModel)) {
        std::snprintf(err, errlen, "%s", j->e.hp.error.c_str());
        delete j;
        return nullptr;
    }
    j->bind();
    return j;
}
void emuljvp_destroy(void* h) { delete (EmulJvp*)h; }
int emuljvp_linearize(void* h, const double* m, int precond, double tol, int maxit) {
    ((EmulJvp*)h)->linearize(m, precond, tol, maxit);
    return 0;
}
int emuljvp_jvp(void* h, const double* v, int wrt, int precond, double tol, int maxit, double* Jv) {
    return ((EmulJvp*)h)->jvp(v, wrt, precond, tol, maxit, Jv);
}
int emuljvp_jtvp(void* h, const double* u, int wrt, int precond, double tol, int maxit, double* JTu) {
    return ((EmulJvp*)h)->jtvp(u, wrt, precond, tol, maxit, JTu);
}

}  // extern "C"
