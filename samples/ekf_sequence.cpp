// ekf_sequence -- the reference's sample program (kalmanFilter/samples/EKF/main.cpp:45-160) on the MI355X engine:
//     ekf_sequence config.yml imgdir/ [outdir/ [first [last [detector_threshold [f32]]]]] [--warp-templates] [--subpixel] [--wide-search] [--patch-normals] [--ncc-distinct COEF] [--consistency] [--budget K] [--position-fixes FILE] [--fixed-map-from FRAME] [--convert-all] [--timestamps FILE [--time-unit SECONDS]] [--save-map FILE] [--load-map FILE] [--iterations K [--iteration-tol T]] [--relocalise LOST_BELOW,LOST_FRAMES (keypoint matcher; with --load-map: relocalises on the first frame)]
// reads imgdir/%05d.png from `first` (default 0; the reference hard-codes 90..6550) until `last` or the first missing
// file, initialises the filter on the first frame, steps on the rest and, when outdir is given, writes
// outdir/output.yml, log.txt and the prediction images in the reference's layout and, after the last frame, outdir/map.ply:
// the map as 3-D points with their standard deviations (ImageEKF::writeMapPly).  Matcher mode B (NCC templates), so no
// OpenCV is needed.  --warp-templates (anywhere after imgdir/): the templates are re-rendered from the predicted viewpoint before
// every search (ImageEKF::setTemplateWarp).  --subpixel (likewise): NCC matches at sub-pixel positions (ImageEKF::setSubpixelMatches).
// --wide-search (likewise): gates larger than the coarse search window are searched whole (ImageEKF::setWideSearch).
// --patch-normals (likewise; implies --warp-templates): the normals of the warp's patches are estimated from the images
// (ImageEKF::setPatchNormals) and map.ply carries them as nx ny nz.
// --ncc-distinct COEF (likewise): an NCC match with a second place in its gate is kept only if its distance is below COEF times
// the rival's, 0 < COEF <= 1 (ImageEKF::setNccDistinct).
// --consistency (likewise): every covariance update records its normalised innovation squared on the device
// (ImageEKF::setConsistency); after each frame one line frame,stage,matches,rows,nis per update is appended to
// outdir/consistency.csv, and after the last frame total NIS / total rows is printed (1 for a consistent filter).
// --budget K (likewise): a step measures at most the K most informative of the features it predicts (ImageEKF::setMeasurementBudget);
// after each frame the predicted and the selected count are printed and appended to outdir/log.txt.
// --position-fixes FILE (likewise): fixes of the camera position from outside the filter (mocap, GPS, odometry), one per line as
// "frame x y z sigma" (# starts a comment; frame = the number in the step line); after that frame's step the fix is fused with
// R = sigma^2 I and no gate (ImageEKF::fuseCameraPosition) and its NIS is printed under the step line.
// --fixed-map-from FRAME (likewise): map as always up to FRAME, then localise -- from the step that prints "step FRAME" on the map
// is fixed (ImageEKF::setFixedMap): both updates move the camera alone, map management is skipped, "fixed map: on" is printed under
// the step line; the covariance carries over from the mapping frames as it is.
// --convert-all (likewise): every map-management tick converts EVERY inverse-depth feature below the linearity threshold to XYZ
// instead of the reference's one (ImageEKF::setConvertAll); log.txt gains "Converted to depth: K" per tick.
// --timestamps FILE (likewise): one time per frame in seconds, in frame order, one per line (# starts a comment); frame i is stepped
// over dt = (t_i - t_(i-1)) / unit instead of 1 (ImageEKF::setFrameInterval); the interval is printed under the step line and log.txt
// gains "Frame interval: dt = D" per step.  --time-unit SECONDS (default 1): set it to the nominal frame period -- the
// configuration's LinearAccelSD and AngularAccelSD were tuned per frame and then keep their meaning; a frame after k dropped ones
// gets dt = k + 1.  A time that does not increase, or a number of times that differs from the number of frames, is an error
// before the first frame is touched.
// --save-map FILE (likewise): after the last frame the whole filter and map go to FILE (ImageEKF::saveMap: one blob).
// --load-map FILE (likewise): the filter starts from such a file instead of initialising on the first frame, which is then stepped
// on like the others (ImageEKF::loadMap); with --fixed-map-from 0 the run localises on the loaded map from its first step, with
// the templates of the run that saved it.  The modes (--warp-templates, --patch-normals, ...) are not in the file: give them again.
// --iterations K [--iteration-tol T] (likewise): both updates of every step are iterated EKF updates of up to K passes
// (ImageEKF::setUpdateIterations); T > 0 ends an iteration once a pass moved no state by T standard deviations.  Under
// the step line the passes and the last normalised step of each update are printed.
// --relocalise LOST_BELOW,LOST_FRAMES (likewise): the run uses the keypoint matcher (detector + BRIEF-32, the detector threshold is
// detector_threshold) and recovers from tracking loss: after LOST_FRAMES consecutive steps with fewer than LOST_BELOW inliers the next
// step first relocalises on its image (ImageEKF::setRelocalise, DESIGN.md 4.17: global descriptor match + P3P RANSAC on the map) and
// "relocalised: ..." or "relocalise failed" is printed above its step line.  With --load-map AND --relocalise the first frame is
// relocalised on once before it is stepped on, so a session may start anywhere in the mapped room.  --load-map alone does not
// relocalise: the relocalisation matches BRIEF-32 descriptors, so it needs the keypoint matcher that --relocalise selects and a map
// that was saved by a run with --relocalise (an NCC-template map has no descriptors to match).
//
//   g++ -std=c++11 -O2 samples/ekf_sequence.cpp -o ekf_sequence -Lopenekfmonoslam_amd -lekf_engine -lz
//   (plus -Wl,-rpath,$PWD/openekfmonoslam_amd -Wl,-rpath,/opt/rocm/lib)
#include <cstdio>
#include <cstdlib>

#include "../openekfmonoslam_amd/compat/ekf_io.h"

struct PositionFix {
    int frame;
    double r[3], sigma;
};

// "frame x y z sigma" per line; # starts a comment, empty lines are skipped
static void readPositionFixes(const std::string &path, std::vector<PositionFix> &fixes)
{
    std::FILE *f = std::fopen(path.c_str(), "r");
    if (!f) throw std::runtime_error("cannot read " + path);
    char line[512];
    for (int no = 1; std::fgets(line, sizeof(line), f); ++no) {
        std::string text(line);
        text = text.substr(0, text.find('#'));
        if (text.find_first_not_of(" \t\r\n") == std::string::npos) continue;
        PositionFix p;
        if (std::sscanf(text.c_str(), "%d %lf %lf %lf %lf", &p.frame, &p.r[0], &p.r[1], &p.r[2], &p.sigma) != 5 || !(p.sigma > 0.0)) {
            std::fclose(f);
            char where[32];
            std::snprintf(where, sizeof(where), ":%d", no);
            throw std::runtime_error(path + where + ": expected \"frame x y z sigma\" with sigma > 0");
        }
        fixes.push_back(p);
    }
    std::fclose(f);
}

int main(int argc, const char *argv[])
{
    bool warp = false, subpix = false, wide = false, normals = false, consistency = false, convertAll = false; // the flags are taken out of the argument list; the positional arguments keep their places
    double distinct = 0.0;
    int budget = 0, fixedFrom = -1, iterations = 1, lostBelow = -1, lostFrames = 0; // lostFrames > 0: --relocalise
    double iterationTol = 0.0;
    std::string fixesFile, timesFile, saveMapFile, loadMapFile;
    double timeUnit = 1.0;
    for (int i = 1; i < argc; ++i)
        if ((std::string(argv[i]) == "--ncc-distinct" || std::string(argv[i]) == "--budget" || std::string(argv[i]) == "--position-fixes" ||
             std::string(argv[i]) == "--fixed-map-from" || std::string(argv[i]) == "--timestamps" || std::string(argv[i]) == "--time-unit" ||
             std::string(argv[i]) == "--save-map" || std::string(argv[i]) == "--load-map" || std::string(argv[i]) == "--iterations" ||
             std::string(argv[i]) == "--iteration-tol" || std::string(argv[i]) == "--relocalise") &&
            i + 1 < argc) { // the flag and its value
            if (std::string(argv[i]) == "--budget") budget = std::atoi(argv[i + 1]);
            else if (std::string(argv[i]) == "--iterations") iterations = std::atoi(argv[i + 1]);
            else if (std::string(argv[i]) == "--iteration-tol") iterationTol = std::atof(argv[i + 1]);
            else if (std::string(argv[i]) == "--relocalise") {
                if (std::sscanf(argv[i + 1], "%d,%d", &lostBelow, &lostFrames) != 2 || lostBelow < 0 || lostFrames < 1) {
                    std::fprintf(stderr, "%s: --relocalise wants LOST_BELOW,LOST_FRAMES (>= 0, >= 1)\n", argv[0]);
                    return 2;
                }
            }
            else if (std::string(argv[i]) == "--timestamps") timesFile = argv[i + 1];
            else if (std::string(argv[i]) == "--save-map") saveMapFile = argv[i + 1];
            else if (std::string(argv[i]) == "--load-map") loadMapFile = argv[i + 1];
            else if (std::string(argv[i]) == "--time-unit") timeUnit = std::atof(argv[i + 1]);
            else if (std::string(argv[i]) == "--fixed-map-from") fixedFrom = std::max(std::atoi(argv[i + 1]), 0);
            else if (std::string(argv[i]) == "--position-fixes") fixesFile = argv[i + 1];
            else distinct = std::atof(argv[i + 1]);
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            --i;
        } else if (std::string(argv[i]) == "--warp-templates" || std::string(argv[i]) == "--subpixel" || std::string(argv[i]) == "--wide-search" ||
            std::string(argv[i]) == "--patch-normals" || std::string(argv[i]) == "--consistency" || std::string(argv[i]) == "--convert-all") {
            if (std::string(argv[i]) == "--patch-normals") normals = true;
            if (std::string(argv[i]) == "--convert-all") convertAll = true;
            else if (std::string(argv[i]) == "--consistency") consistency = true;
            else (std::string(argv[i]) == "--subpixel" ? subpix : std::string(argv[i]) == "--wide-search" ? wide : warp) = true;
            for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
            --argc;
            --i;
        }
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s config.yml imgdir/ [outdir/ [first [last [detector_threshold [f32]]]]] [--warp-templates] [--subpixel] [--wide-search] [--patch-normals] [--ncc-distinct COEF] [--consistency] [--budget K] [--position-fixes FILE] [--fixed-map-from FRAME] [--convert-all] [--timestamps FILE [--time-unit SECONDS]] [--save-map FILE] [--load-map FILE] [--iterations K [--iteration-tol T]] [--relocalise LOST_BELOW,LOST_FRAMES (keypoint matcher; with --load-map: relocalises on the first frame)]\n", argv[0]);
        return 2;
    }
    const std::string outputPath = argc > 3 ? argv[3] : "";
    const int first = argc > 4 ? std::atoi(argv[4]) : 0, last = argc > 5 ? std::atoi(argv[5]) : 99999;
    const double threshold = argc > 6 ? std::atof(argv[6]) : 1e9;
    const int precision = (argc > 7 && std::string(argv[7]) == "f32") ? EKF_PRECISION_F32 : EKF_PRECISION_F64;
    try {
        ekf_compat::FileSequenceImageGenerator generator(argv[2], "", "png", first, last);
        generator.init();
        std::vector<double> intervals; // per frame, with --timestamps (checked against the frames on disk before any is read)
        if (!timesFile.empty()) ekf_compat::readFrameIntervals(timesFile, timeUnit, generator.remaining(), intervals);
        ekf_compat::Image image = generator.getNextImage();
        if (image.empty()) {
            std::printf("No se puede iniciar Kalman Filter dado que no hay imagenes disponibles.\n");
            return 0;
        }
        if (precision == EKF_PRECISION_F64 && threshold == 1e9 && !warp && !subpix && !wide && distinct == 0.0 && !consistency && budget == 0 && fixesFile.empty() && fixedFrom < 0 && !convertAll && timesFile.empty() && saveMapFile.empty() && loadMapFile.empty() && iterations == 1 && lostFrames == 0) {
            // the reference's own three lines (samples/EKF/main.cpp:76-131): EKF(config, outputPath), init(image), step(image)
            EKF extendedKalmanFilter(argv[1], outputPath.c_str());
            extendedKalmanFilter.init(ekf_compat::matFromImage(image));
            std::printf("init: %d features\n", (int)extendedKalmanFilter.state.mapFeatures.size());
            image = generator.getNextImage();
            int steps = 0;
            while (!image.empty()) {
                extendedKalmanFilter.step(ekf_compat::matFromImage(image));
                const EkfStepInfo &info = extendedKalmanFilter.lastStepInfo();
                const double *x = extendedKalmanFilter.state.position;
                std::printf("step %d: predicted %d matches %d li %d hi %d features %d  r = %.6f %.6f %.6f\n", ++steps, info.n_predicted,
                            info.n_matches, info.n_inliers, info.n_rescued, (int)extendedKalmanFilter.state.mapFeatures.size(), x[0], x[1], x[2]);
                image = generator.getNextImage();
            }
            if (!outputPath.empty()) ekf_compat::writeMapPly(extendedKalmanFilter.engine(), outputPath + "map.ply");
            return 0;
        }
        // (a detector threshold, the fp32 configuration, the template warp, sub-pixel matches, the wide search, the distinctiveness test, the consistency records, a measurement budget, position fixes, a fixed map, the batch conversion, frame times or a map file asked for: the driver class with its extra arguments)
        ekf_compat::ImageEKF extendedKalmanFilter(argv[1], outputPath.c_str(), precision, threshold,
                                                  lostFrames > 0 ? EKF_IMAGE_MATCHER_KEYPOINTS : EKF_IMAGE_MATCHER_NCC, threshold);
        EkfRelocParams reloc = EkfRelocParams();
        reloc.hypotheses = 256; reloc.min_inliers = 8; reloc.seed = 1;
        reloc.max_distance = 48.0; reloc.second_best_coef = 0.8; reloc.inlier_px = 3.0; reloc.max_rel_depth_sd = 0.3;
        reloc.sigma_position = 0.05; reloc.sigma_angle = 0.02; reloc.install = 1;
        if (lostFrames > 0) extendedKalmanFilter.setRelocalise(lostBelow, lostFrames, reloc);
        extendedKalmanFilter.setTemplateWarp(warp);
        if (normals) extendedKalmanFilter.setPatchNormals(true);
        extendedKalmanFilter.setSubpixelMatches(subpix);
        extendedKalmanFilter.setWideSearch(wide);
        extendedKalmanFilter.setNccDistinct(distinct);
        extendedKalmanFilter.setConsistency(consistency);
        extendedKalmanFilter.setMeasurementBudget(budget);
        extendedKalmanFilter.setConvertAll(convertAll);
        if (iterations != 1 || iterationTol != 0.0) extendedKalmanFilter.setUpdateIterations(iterations, iterationTol);
        std::vector<PositionFix> fixes;
        if (!fixesFile.empty()) readPositionFixes(fixesFile, fixes);
        std::FILE *csv = 0;
        if (consistency && !outputPath.empty() && !(csv = std::fopen((outputPath + "consistency.csv").c_str(), "w")))
            throw std::runtime_error("cannot write " + outputPath + "consistency.csv");
        if (loadMapFile.empty()) {
            extendedKalmanFilter.init(image);
            std::printf("init: %d features\n", ekf_num_features(extendedKalmanFilter.engine()));
            image = generator.getNextImage();
        } else { // the first frame is a step like the others
            const EkfMapBlobInfo info = extendedKalmanFilter.loadMap(loadMapFile);
            std::printf("loaded map: %d features, %llu bytes\n", info.N, (unsigned long long)info.total_bytes);
            if (lostFrames > 0) { // the session may start anywhere on the loaded map
                const EkfRelocResult res = extendedKalmanFilter.relocalise(image, reloc);
                if (res.found) std::printf("relocalised: inliers %d of %d candidates, rms %.3f px\n", res.n_inliers, res.n_candidates, res.rms_px);
                else std::printf("relocalise failed: %d candidates, best %d inliers\n", res.n_candidates, res.n_inliers);
            }
        }
        while (!image.empty()) {
            if (fixedFrom >= 0 && extendedKalmanFilter.steps() + 1 >= fixedFrom && !extendedKalmanFilter.fixedMap()) extendedKalmanFilter.setFixedMap(true);
            if (!intervals.empty()) extendedKalmanFilter.setFrameInterval(intervals[(size_t)extendedKalmanFilter.steps() + 1]);
            const bool relocDue = lostFrames > 0 && extendedKalmanFilter.lostRun() >= lostFrames; // this step relocalises first
            const EkfStepInfo info = extendedKalmanFilter.step(image);
            if (relocDue) {
                const EkfRelocResult &res = extendedKalmanFilter.lastRelocalise();
                if (res.found) std::printf("relocalised: inliers %d of %d candidates, rms %.3f px\n", res.n_inliers, res.n_candidates, res.rms_px);
                else std::printf("relocalise failed: %d candidates, best %d inliers\n", res.n_candidates, res.n_inliers);
            }
            double x[13];
            ekf_get_state(extendedKalmanFilter.engine(), x, 0, 0);
            std::printf("step %d: predicted %d matches %d li %d hi %d features %d  r = %.6f %.6f %.6f\n", extendedKalmanFilter.steps(),
                        info.n_predicted, info.n_matches, info.n_inliers, info.n_rescued, ekf_num_features(extendedKalmanFilter.engine()),
                        x[0], x[1], x[2]);
            if (extendedKalmanFilter.fixedMap()) std::printf("        fixed map: on\n");
            if (iterations > 1) {
                std::vector<EkfIterationRecord> recs;
                extendedKalmanFilter.iterationRecords(recs);
                for (size_t k = 0; k < recs.size(); ++k)
                    std::printf("        iterated update %d: passes %d stop %d last step %.3g\n", recs[k].stage, recs[k].passes_run, recs[k].stop_reason,
                                recs[k].passes_run > 0 ? recs[k].step[recs[k].passes_run - 1] : 0.0);
            }
            if (!intervals.empty()) std::printf("        frame interval: dt = %g\n", extendedKalmanFilter.frameInterval());
            for (size_t k = 0; k < fixes.size(); ++k)
                if (fixes[k].frame == extendedKalmanFilter.steps()) {
                    const double s2 = fixes[k].sigma * fixes[k].sigma, R[9] = {s2, 0, 0, 0, s2, 0, 0, 0, s2};
                    const EkfExternalUpdate fix = extendedKalmanFilter.fuseCameraPosition(fixes[k].r, R);
                    std::printf("        position fix: nis %.6f\n", fix.nis);
                }
            if (warp) {
                int warped = 0, fallback = 0;
                ekf_get_template_warp_counts(extendedKalmanFilter.engine(), &warped, &fallback);
                std::printf("        template levels warped %d, fallen back %d\n", warped, fallback);
            }
            if (normals) {
                int updated = 0, skipped = 0;
                ekf_get_patch_normal_counts(extendedKalmanFilter.engine(), &updated, &skipped);
                std::printf("        patch normals updated %d, skipped %d\n", updated, skipped);
            }
            if (subpix) {
                int refined = 0, integer = 0;
                ekf_get_subpixel_counts(extendedKalmanFilter.engine(), &refined, &integer);
                std::printf("        match axes refined %d, left at the integer %d\n", refined, integer);
            }
            if (wide) {
                int slots = 0, cands = 0;
                ekf_get_ncc_wide_counts(extendedKalmanFilter.engine(), &slots, &cands);
                std::printf("        gates searched wide %d, coarse candidates %d\n", slots, cands);
            }
            if (distinct != 0.0) {
                int with_rival = 0, rejected = 0;
                ekf_get_ncc_distinct_counts(extendedKalmanFilter.engine(), &with_rival, &rejected);
                std::printf("        matches with a rival in the gate %d, rejected %d\n", with_rival, rejected);
            }
            if (budget > 0) {
                int predicted = 0, selected = 0;
                ekf_get_measurement_budget_counts(extendedKalmanFilter.engine(), &predicted, &selected);
                std::printf("        measurement budget: predicted %d selected %d\n", predicted, selected);
            }
            if (consistency) {
                std::vector<EkfUpdateConsistency> recs;
                extendedKalmanFilter.consistency(recs);
                for (size_t k = 0; k < recs.size(); ++k) {
                    std::printf("        update stage %d: matches %d rows %d nis %.6f\n", recs[k].stage, recs[k].matches, recs[k].rows, recs[k].nis);
                    if (csv) std::fprintf(csv, "%d,%d,%d,%d,%.17g\n", extendedKalmanFilter.steps(), recs[k].stage, recs[k].matches, recs[k].rows, recs[k].nis);
                }
            }
            image = generator.getNextImage();
        }
        if (consistency) {
            double nis = 0.0;
            int64_t rows = 0, updates = 0;
            ekf_get_consistency_totals(extendedKalmanFilter.engine(), &nis, &rows, &updates);
            std::printf("consistency: %lld updates, total NIS %.6f / total rows %lld = %.6f\n", (long long)updates, nis, (long long)rows,
                        rows > 0 ? nis / (double)rows : 0.0);
            if (csv && std::fclose(csv) != 0) throw std::runtime_error("cannot write " + outputPath + "consistency.csv");
        }
        if (!outputPath.empty()) extendedKalmanFilter.writeMapPly(outputPath + "map.ply");
        if (!saveMapFile.empty()) {
            extendedKalmanFilter.saveMap(saveMapFile);
            std::printf("saved map: %d features to %s\n", ekf_num_features(extendedKalmanFilter.engine()), saveMapFile.c_str());
        }
    } catch (const std::exception &ex) {
        std::fprintf(stderr, "ekf_sequence: %s\n", ex.what());
        return 1;
    }
    return 0;
}
