// The views-solver slice of csrc/k_triangulate.hip with the lowest observing view as the anchor (mv_stage_pose, mv_track<true>; sliced out of
// the product source behind the two-view slice and the shared geometry of csrc/twoview_math.hpp by tests/test_tracks_emulated.py into
// tracks_anchor_slice.hpp) on the host, and the reference instantiation (mv_stage_view, mv_track<false>) on the same tracks.
// stdin: G int32, then per scene fp64: V, nv, m, min_views, thr2, cos_min, max_depth, V x (R (9), t (3), K (9)), m x V x (u, v, in range 0 / 1)
// stdout: per track status, n_inliers, inlier mask, winner int32 (all scenes), then X (3), err fp32, then score, cost0, cost1 fp64 of
// mv_track<true>; then the same three blocks of mv_track<false>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define __device__
namespace xfh {
using std::fabs;
using std::floor;
using std::sqrt;
#include "tracks_anchor_slice.hpp"
}  // namespace xfh
struct HostObs {
    const double* p;          // V x (u, v, in range)
    bool operator()(int w, double& u, double& v) const {
        const bool in = p[3 * w + 2] != 0.0;
        u = in ? p[3 * w] : (double)NAN;
        v = in ? p[3 * w + 1] : (double)NAN;
        return in;
    }
};
struct Out {
    std::vector<int32_t> iv;
    std::vector<float> fv;
    std::vector<double> dv;
    void add(const xfh::MvResult& r) {
        iv.insert(iv.end(), {r.status, r.n_inliers, (int32_t)r.inliers, r.winner});
        fv.insert(fv.end(), {r.X[0], r.X[1], r.X[2], r.err});
        dv.insert(dv.end(), {r.score, r.cost0, r.cost1});
    }
    void write() const {
        fwrite(iv.data(), 4, iv.size(), stdout);
        fwrite(fv.data(), 4, fv.size(), stdout);
        fwrite(dv.data(), 8, dv.size(), stdout);
    }
};
int main() {
    int G = 0;
    if (fread(&G, 4, 1, stdin) != 1) return 2;
    Out anchored, reference;
    for (int g = 0; g < G; ++g) {
        double hdr[7];
        if (fread(hdr, 8, 7, stdin) != 7) return 2;
        const int V = (int)hdr[0], nv = (int)hdr[1], m = (int)hdr[2], min_views = (int)hdr[3];
        if (V < 1 || V > xfh::mv::MAX_VIEWS || nv > V || m < 0) return 3;
        std::vector<double> cam((size_t)V * 21), obs((size_t)m * V * 3), va((size_t)V * xfh::mv::STRIDE, (double)NAN), vr((size_t)V * xfh::mv::STRIDE);
        if (fread(cam.data(), 8, cam.size(), stdin) != cam.size() || fread(obs.data(), 8, obs.size(), stdin) != obs.size()) return 2;
        for (int v = 0; v < V; ++v) {       // (va keeps NaN in the fields of a fixed reference view: mv_track<true> does not read them)
            xfh::mv_stage_pose(&cam[(size_t)v * 21], &cam[(size_t)v * 21 + 9], &cam[(size_t)v * 21 + 12], &va[(size_t)v * xfh::mv::STRIDE]);
            xfh::mv_stage_view(&cam[(size_t)v * 21], &cam[(size_t)v * 21 + 9], &cam[(size_t)v * 21 + 12], &cam[0], &cam[9], &vr[(size_t)v * xfh::mv::STRIDE]);
        }
        for (int k = 0; k < m; ++k) {
            HostObs o{&obs[(size_t)k * V * 3]};
            anchored.add(xfh::mv_track<true>(va.data(), nv, o, hdr[4], hdr[5], hdr[6], min_views));
            reference.add(xfh::mv_track<false>(vr.data(), nv, o, hdr[4], hdr[5], hdr[6], min_views));
        }
    }
    anchored.write();
    reference.write();
    return 0;
}
