// wide_search_check -- ekf_compat::ImageEKF over a PNG sequence with ImageEKF::setWideSearch(true): every step has to return
// EKF_OK, printed one line per step with the wide counts; then the covariance is inflated (P x 400: gates 20 times as wide),
// the last frame is matched from that state through the C ABI with the mode off, on (set through the driver class) and
// on (set through ekf_set_ncc_wide_search), and the two mode-on match lists have to be the same bytes with wide slots counted.
//     wide_search_check config.yml imgdir/ detector_threshold
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../openekfmonoslam_amd/compat/ekf_io.h"

static int match(EkfEngine *e, std::vector<EkfMatch> &m, int *slots, int *cands)
{
    int np = 0, n = 0;
    if (ekf_predict_measurements(e, 0, 0, 0, &np, 0, 0) != EKF_OK) return -1;
    m.assign(ekf_num_features(e) + 1, EkfMatch());
    if (ekf_match_ncc(e, m.data(), &n) != EKF_OK) return -1;
    if (ekf_get_ncc_wide_counts(e, slots, cands) != EKF_OK) return -1;
    m.resize(n);
    return n;
}

int main(int argc, const char *argv[])
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s config.yml imgdir/ detector_threshold\n", argv[0]);
        return 2;
    }
    try {
        ekf_compat::FileSequenceImageGenerator generator(argv[2], "", "png", 0, 99999);
        generator.init();
        ekf_compat::Image image = generator.getNextImage();
        if (image.empty()) {
            std::fprintf(stderr, "no frames in %s\n", argv[2]);
            return 2;
        }
        ekf_compat::ImageEKF ekf(argv[1], "", EKF_PRECISION_F64, std::atof(argv[3]));
        ekf.setWideSearch(true);
        ekf.init(image);
        EkfEngine *e = ekf.engine();
        for (image = generator.getNextImage(); !image.empty(); image = generator.getNextImage()) {
            const EkfStepInfo info = ekf.step(image);
            int slots = -1, cands = -1;
            const int rc = ekf_get_ncc_wide_counts(e, &slots, &cands);
            std::printf("step %d status %d matches %d wide %d candidates %d\n", ekf.steps(), info.status, info.n_matches, slots, cands);
            if (rc != EKF_OK || info.status != EKF_OK || slots < 0 || cands < 0) return 1;
        }
        // the last frame is still on the device: inflate P and match it three ways
        const int n = ekf_state_dim(e), N = ekf_num_features(e);
        std::vector<double> x(13), fp(6 * (size_t)N), P((size_t)n * n);
        std::vector<int32_t> type(N), covpos(N);
        if (ekf_get_state(e, x.data(), fp.data(), P.data()) != EKF_OK || ekf_get_feature_layout(e, type.data(), covpos.data()) != EKF_OK) return 1;
        for (size_t i = 0; i < P.size(); ++i) P[i] *= 400.0;
        if (ekf_set_state(e, x.data(), N, fp.data(), type.data(), 0, P.data()) != EKF_OK) return 1;
        std::vector<EkfMatch> off, on_class, on_abi;
        int s0 = -1, c0 = -1, s1 = -1, c1 = -1, s2 = -1, c2 = -1;
        ekf.setWideSearch(false);
        const int n_off = match(e, off, &s0, &c0);
        ekf.setWideSearch(true);
        const int n_class = match(e, on_class, &s1, &c1);
        if (ekf_set_ncc_wide_search(e, 0) != EKF_OK || ekf_set_ncc_wide_search(e, 1) != EKF_OK) return 1;
        const int n_abi = match(e, on_abi, &s2, &c2);
        std::printf("match off %d wide %d candidates %d\n", n_off, s0, c0);
        std::printf("match class %d wide %d candidates %d\n", n_class, s1, c1);
        std::printf("match abi %d wide %d candidates %d\n", n_abi, s2, c2);
        if (n_off < 0 || n_class < 0 || n_abi < 0) return 1;
        if (s0 != 0 || c0 != 0 || s1 <= 0 || c1 <= 0 || s1 != s2 || c1 != c2 || n_class != n_abi) return 1;
        if (n_class > 0 && std::memcmp(on_class.data(), on_abi.data(), (size_t)n_class * sizeof(EkfMatch)) != 0) return 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
