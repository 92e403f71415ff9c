// subpixel_check -- ekf_compat::ImageEKF over a PNG sequence with ImageEKF::setSubpixelMatches(true): every step has to
// return EKF_OK and report two axes per match (refined + integer), printed one line per step; then the last frame is
// matched once more from the final state and the axes of its matches that are not at an integer pixel are counted.
//     subpixel_check config.yml imgdir/ detector_threshold
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../openekfmonoslam_amd/compat/ekf_io.h"

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
        ekf.setSubpixelMatches(true);
        ekf.init(image);
        for (image = generator.getNextImage(); !image.empty(); image = generator.getNextImage()) {
            const EkfStepInfo info = ekf.step(image);
            int refined = -1, integer = -1;
            const int rc = ekf_get_subpixel_counts(ekf.engine(), &refined, &integer);
            std::printf("step %d status %d matches %d refined %d integer %d\n", ekf.steps(), info.status, info.n_matches, refined, integer);
            if (rc != EKF_OK || info.status != EKF_OK || refined + integer != 2 * info.n_matches) {
                std::fprintf(stderr, "step %d: status %d, counts %d + %d for %d matches\n", ekf.steps(), info.status, refined, integer,
                             info.n_matches);
                return 1;
            }
        }
        // the last frame is still on the device
        EkfEngine *e = ekf.engine();
        int np = 0, n = 0, off_integer = 0;
        if (ekf_predict_measurements(e, 0, 0, 0, &np, 0, 0) != EKF_OK) return 1;
        std::vector<EkfMatch> matches(ekf_num_features(e) + 1);
        if (ekf_match_ncc(e, matches.data(), &n) != EKF_OK) return 1;
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 2; ++a)
                if (matches[i].imagePos[a] != std::floor(matches[i].imagePos[a])) ++off_integer;
        std::printf("match %d axes_off_integer %d of %d\n", n, off_integer, 2 * n);
        if (n <= 0 || off_integer == 0) return 1;
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
