// external_update_check -- external measurements through the C++ driver classes over a PNG sequence (NCC matcher, as
// samples/ekf_sequence.cpp drives it):
//   1. two ekf_compat::ImageEKF runs over the same frames in the reproducible sweep mode; one fuses a position fix with
//      ImageEKF::fuseCameraPosition, the other with the C ABI's ekf_fuse_camera_position: same record, same x, features and P,
//      bit for bit; likewise ImageEKF::fuseFeatureDistance and ImageEKF::updateExternal against their C entries;
//   2. class EKF under the reference's own signatures: after EKF::fuseCameraPosition the public attributes are the updated
//      ones -- `state` at once, `stateCovarianceMatrix` on first access -- and equal what the engine holds.
//     external_update_check config.yml imgdir/ detector_threshold
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../openekfmonoslam_amd/compat/ekf_io.h"

static void fail(const char *what)
{
    std::fprintf(stderr, "external_update_check: %s\n", what);
    std::exit(1);
}

struct Snapshot {
    double x[13];
    std::vector<double> fp, P;
};

static Snapshot snapshot(EkfEngine *e)
{
    Snapshot s;
    const int N = ekf_num_features(e), n = ekf_state_dim(e);
    s.fp.assign(6 * (size_t)N + 6, 0.0);
    s.P.assign((size_t)n * n, 0.0);
    if (ekf_get_state(e, s.x, s.fp.data(), s.P.data()) != EKF_OK) fail("ekf_get_state");
    return s;
}

static bool same(const Snapshot &a, const Snapshot &b)
{
    return std::memcmp(a.x, b.x, sizeof(a.x)) == 0 && a.fp.size() == b.fp.size() && a.P.size() == b.P.size() &&
           std::memcmp(a.fp.data(), b.fp.data(), a.fp.size() * sizeof(double)) == 0 &&
           std::memcmp(a.P.data(), b.P.data(), a.P.size() * sizeof(double)) == 0;
}

static bool same(const EkfExternalUpdate &a, const EkfExternalUpdate &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static void run(ekf_compat::ImageEKF &ekf, const char *imgdir)
{
    ekf_compat::FileSequenceImageGenerator generator(imgdir, "", "png", 0, 99999);
    generator.init();
    ekf_compat::Image image = generator.getNextImage();
    if (image.empty()) fail("no frames");
    if (ekf_set_sweep_mode(ekf.engine(), EKF_SWEEP_LAUNCHES) != EKF_OK) fail("ekf_set_sweep_mode");
    ekf.init(image);
    for (image = generator.getNextImage(); !image.empty(); image = generator.getNextImage()) ekf.step(image);
}

int main(int argc, const char *argv[])
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s config.yml imgdir/ detector_threshold\n", argv[0]);
        return 2;
    }
    try {
        const double R[9] = {2e-4, 5e-5, 2e-5, 5e-5, 1.5e-4, -3e-5, 2e-5, -3e-5, 1e-4};
        {
            ekf_compat::ImageEKF a(argv[1], "", EKF_PRECISION_F64, std::atof(argv[3])), b(argv[1], "", EKF_PRECISION_F64, std::atof(argv[3]));
            run(a, argv[2]);
            run(b, argv[2]);
            if (a.steps() != 7 || ekf_num_features(a.engine()) < 2) fail("the sequence did not run");
            Snapshot before = snapshot(a.engine());
            if (!same(before, snapshot(b.engine()))) fail("two runs of the same frames differ");
            // a position fix
            const double r[3] = {before.x[0] + 0.003, before.x[1] - 0.002, before.x[2] + 0.001};
            const EkfExternalUpdate ua = a.fuseCameraPosition(r, R);
            EkfExternalUpdate ub;
            if (ekf_fuse_camera_position(b.engine(), r, R, 0.0, &ub) != EKF_OK) fail("ekf_fuse_camera_position");
            if (!ua.applied || ua.rows != 3 || !(ua.nis > 0.0) || !same(ua, ub)) fail("ImageEKF::fuseCameraPosition: not the C ABI's record");
            Snapshot sa = snapshot(a.engine());
            if (same(sa, before) || !same(sa, snapshot(b.engine()))) fail("ImageEKF::fuseCameraPosition: not the C ABI's state");
            std::printf("position fix: nis %.6f\n", ua.nis);
            // a distance between the first and the last feature, 10 % longer than the map has it
            std::vector<EkfMapPoint> pts;
            a.mapPoints(pts);
            const int last = (int)pts.size() - 1;
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (pts[0].xyz[k] - pts[last].xyz[k]) * (pts[0].xyz[k] - pts[last].xyz[k]);
            d = 1.1 * std::sqrt(d);
            const EkfExternalUpdate da = a.fuseFeatureDistance(0, last, d, 1e-3 * d);
            EkfExternalUpdate db;
            if (ekf_fuse_feature_distance(b.engine(), 0, last, d, 1e-3 * d, 0.0, &db) != EKF_OK) fail("ekf_fuse_feature_distance");
            if (!da.applied || da.rows != 1 || !same(da, db) || !same(snapshot(a.engine()), snapshot(b.engine())))
                fail("ImageEKF::fuseFeatureDistance: not the C ABI's result");
            std::printf("distance: nis %.6f\n", da.nis);
            // the generic call: the linear velocity observed directly, gated out and then applied
            const int32_t rowStart[4] = {0, 1, 2, 3}, col[3] = {7, 8, 9};
            const double val[3] = {1.0, 1.0, 1.0}, residual[3] = {1e-3, -1e-3, 2e-3}, Rv[9] = {1e-6, 0, 0, 0, 1e-6, 0, 0, 0, 1e-6};
            sa = snapshot(a.engine());
            const EkfExternalUpdate gated = a.updateExternal(3, rowStart, col, val, residual, Rv, 1e-12);
            if (gated.applied || !same(sa, snapshot(a.engine()))) fail("ImageEKF::updateExternal: a gated-out update changed the filter");
            const EkfExternalUpdate va = a.updateExternal(3, rowStart, col, val, residual, Rv);
            EkfExternalUpdate vb;
            if (ekf_update_external(b.engine(), 3, rowStart, col, val, residual, Rv, 0.0, &vb) != EKF_OK) fail("ekf_update_external");
            if (!va.applied || va.nis != gated.nis || !same(va, vb) || !same(snapshot(a.engine()), snapshot(b.engine())))
                fail("ImageEKF::updateExternal: not the C ABI's result");
            bool threw = false;
            try {
                const double Rbad[9] = {-1e6, 0, 0, 0, -1e6, 0, 0, 0, -1e6};
                a.updateExternal(3, rowStart, col, val, residual, Rbad);
            } catch (const std::exception &) {
                threw = true;
            }
            if (!threw || !same(snapshot(a.engine()), snapshot(b.engine()))) fail("ImageEKF::updateExternal: S not positive definite must throw and change nothing");
        }
        {
            // class EKF, the reference's three lines, then a fix: the public attributes follow
            ekf_compat::FileSequenceImageGenerator generator(argv[2], "", "png", 0, 99999);
            generator.init();
            ekf_compat::Image image = generator.getNextImage();
            EKF ekf(argv[1], "");
            ekf.init(ekf_compat::matFromImage(image));
            for (image = generator.getNextImage(); !image.empty(); image = generator.getNextImage()) ekf.step(ekf_compat::matFromImage(image));
            const Matd &P = ekf.stateCovarianceMatrix;
            const double p00 = P[0][0], r0[3] = {ekf.state.position[0], ekf.state.position[1], ekf.state.position[2]};
            const double r[3] = {r0[0] + 0.003, r0[1] - 0.002, r0[2] + 0.001};
            const EkfExternalUpdate u = ekf.fuseCameraPosition(r, R);
            if (!u.applied) fail("EKF::fuseCameraPosition was not applied");
            if (!P.staleOnHost()) fail("EKF::fuseCameraPosition: stateCovarianceMatrix must be marked stale, as a step marks it");
            const Snapshot s = snapshot(ekf.engine());
            if (std::memcmp(ekf.state.x13(), s.x, sizeof(s.x)) != 0) fail("EKF::fuseCameraPosition: `state` is not the engine's");
            if (ekf.state.position[0] == r0[0]) fail("EKF::fuseCameraPosition: `state` did not move");
            for (size_t i = 0; i < ekf.state.mapFeatures.size(); ++i)
                if (std::memcmp(ekf.state.mapFeatures[i]->position, &s.fp[6 * i], ekf.state.mapFeatures[i]->positionDimension * sizeof(double)) != 0)
                    fail("EKF::fuseCameraPosition: a map feature of `state` is not the engine's");
            const int n = ekf_state_dim(ekf.engine());
            if (P.rows != n || P.cols != n) fail("stateCovarianceMatrix has the wrong size");
            if (std::memcmp(P.ptr(), s.P.data(), s.P.size() * sizeof(double)) != 0) fail("stateCovarianceMatrix is not the engine's after the fix");
            if (!(P[0][0] < p00)) fail("the fix did not shrink the position variance");
        }
        std::printf("external update through the driver class: ok\n");
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
