// relocalise_check -- ekf_compat::ImageEKF::setRelocalise / relocalise with the keypoint matcher over a PNG sequence: init on the
// first frame, then one image step per further frame with the automatic recovery armed so that EVERY step counts as lost
// (lostBelow far above any inlier count) -- after lost_frames such steps the next step relocalises first.  Prints per step the
// counters, the run of lost steps after it and whether the step relocalised, with what it found.
//     relocalise_check config.yml imgdir/ outdir/ new_feature_threshold keypoint_threshold lost_frames
#include <cstdio>
#include <cstdlib>

#include "../../openekfmonoslam_amd/compat/ekf_io.h"

int main(int argc, const char *argv[])
{
    if (argc < 7) {
        std::fprintf(stderr, "usage: %s config.yml imgdir/ outdir/ new_feature_threshold keypoint_threshold lost_frames\n", argv[0]);
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
        ekf_compat::ImageEKF ekf(argv[1], argv[3], EKF_PRECISION_F64, std::atof(argv[4]), EKF_IMAGE_MATCHER_KEYPOINTS, std::atof(argv[5]));
        EkfRelocParams p = EkfRelocParams();
        p.hypotheses = 128; p.min_inliers = 6; p.seed = 3;
        p.max_distance = 40.0; p.second_best_coef = 0.8; p.inlier_px = 3.0; p.max_rel_depth_sd = 0.0;
        p.sigma_position = 0.05; p.sigma_angle = 0.02; p.install = 0;
        const int lostFrames = std::atoi(argv[6]);
        ekf.setRelocalise(1000000, lostFrames, p);
        ekf.init(image);
        std::printf("init %d\n", ekf_num_features(ekf.engine()));
        for (image = generator.getNextImage(); !image.empty(); image = generator.getNextImage()) {
            const bool due = ekf.lostRun() >= lostFrames;
            const EkfStepInfo info = ekf.step(image);
            const EkfRelocResult &r = ekf.lastRelocalise();
            std::printf("step %d inliers %d status %d lost %d relocalised %d found %d installed %d candidates %d hypotheses %d\n", ekf.steps(),
                        info.n_inliers + info.n_rescued, info.status, ekf.lostRun(), due ? 1 : 0, due ? r.found : -1, due ? r.installed : -1,
                        due ? r.n_candidates : -1, due ? r.n_hypotheses : -1);
        }
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "error: %s\n", ex.what());
        return 1;
    }
    return 0;
}
