// The reference's lattice detector (src/SamplePointDetection.cpp, inc/Samplepoint.h,
// the loop of trgt/demo.cpp:206-209,271-276) on include/mvsv_detection.hpp.
//   samplepoint_check cpu OUT_DIR      layout, host decisions, PLY counter
//   samplepoint_check gpu OUT_DIR      + build() on the device, both detectors on a stream
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>

#include "mvsv_stereosystem.hpp"  // also compiles RawDisparityStream's lattice methods

static const mvsv::QMatrix Q = {1.f, 0.f, 0.f, -183.390320f, 0.f, 1.f, 0.f, -120.106110f,
                                0.f, 0.f, 0.f, 303.516571f,  0.f, 0.f, 0.00842495915f, 0.f};

static std::string slurp(const std::string& path)
{
    std::ifstream f(path, std::ios::binary);
    return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

#define REQUIRE(cond, code)                                  \
    do {                                                     \
        if (!(cond)) {                                       \
            std::printf("failed: %s (%d)\n", #cond, code);   \
            return code;                                     \
        }                                                    \
    } while (0)

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    const bool gpu = std::strcmp(argv[1], "gpu") == 0;
    const std::string dir = argv[2];
    try {
        // layout: 100 x 70 -> steps 8 / 8, 11 x 7 points, columns in the outer loop
        mvsv::Mat dmap(70, 100, mvsv::MAT_16SC1);
        for (int y = 0; y < dmap.rows; y++)
            for (int x = 0; x < dmap.cols; x++)
                dmap.ptr<int16_t>(y)[x] = (int16_t)((x * 37 + y * 11) % 23 == 0 ? -16 : (x * 7 + y * 3) % 900);
        mvsv::SamplepointDetection d(dir);
        d.init(dmap, Q, 0.1f, 1.5f);
        int sx, sy, nx, ny;
        REQUIRE(mvsv_samplepoint_layout(100, 70, &sx, &sy, &nx, &ny) == MVSV_OK, 10);
        REQUIRE(sx == 8 && sy == 8 && nx == 11 && ny == 7, 11);
        const auto& sp = d.getSamplepointVec();
        REQUIRE(sp.size() == 77, 12);
        REQUIRE(sp[0].center.x == 8 && sp[0].center.y == 8 && sp[1].center.x == 8 && sp[1].center.y == 16, 13);
        REQUIRE(sp[7].center.x == 16 && sp[7].center.y == 8 && sp[76].center.x == 88 && sp[76].center.y == 56, 14);
        REQUIRE(sp[0].radius == 2 && sp[0].roi.x == 6 && sp[0].roi.y == 6 && sp[0].roi.width == 5, 15);
        REQUIRE(d.getFoundObstacles().size() == 77, 16);  // the layout until the first detectObstacles
        d.setRange(0.9f, 2.7f);
        REQUIRE(d.getRange().first == 0 && d.getRange().second == 2, 17);
        REQUIRE(mvsv_samplepoint_layout(15, 100, &sx, &sy, &nx, &ny) == MVSV_OK && nx * ny == 0, 18);
        {  // hit records need build()'s values first
            bool refused = false;
            const mvsv_sample_hit h{0, 0.f, 0.f, 0.f};
            try {
                d.detectObstacles(1, &h);
            } catch (const mvsv::Error& e) {
                refused = e.code() == MVSV_E_INVALID_ARG;
            }
            REQUIRE(refused && d.getFoundObstacles().size() == 77, 19);
        }
        // host decisions on supplied values: bounds excluded, points as calcCoordinate
        const std::pair<float, float> range = d.getRangeDisparity();
        std::vector<float> vals(77);
        for (int i = 0; i < 77; i++) vals[i] = range.second - 20.f + (range.first - range.second + 40.f) * i / 76.f;
        vals[3] = range.first;
        vals[4] = range.second;
        d.build(dmap, 0, 0, vals.data());
        d.detectObstacles();
        size_t k = 0;
        for (int i = 0; i < 77; i++) {
            if (!(vals[i] < range.first && vals[i] > range.second)) continue;
            REQUIRE(k < d.getFoundObstacles().size(), 20);
            const mvsv::Samplepoint& s = d.getFoundObstacles()[k];
            REQUIRE(s.center.x == sp[i].center.x && s.center.y == sp[i].center.y && s.value == vals[i], 21);
            const auto c = mvsv::Utility::calcCoordinate({vals[i], (float)s.center.x, (float)s.center.y}, Q);
            REQUIRE(std::memcmp(c.data(), d.getFoundPoints()[k].data(), 16) == 0, 22);
            k++;
        }
        REQUIRE(k == d.getFoundObstacles().size() && k > 10, 23);
        REQUIRE(d.getObstacleCounter() == 1 && !slurp(dir + "/pcl_0000.ply").empty(), 24);
        // the same decisions handed in as hit records: same points, same file
        std::vector<mvsv_sample_hit> rec;
        for (int i = 0; i < 77; i++)
            if (vals[i] < range.first && vals[i] > range.second) {
                const auto c = mvsv::Utility::calcCoordinate({vals[i], (float)sp[i].center.x, (float)sp[i].center.y}, Q);
                rec.push_back({i, c[0], c[1], c[2]});
            }
        const std::vector<std::array<float, 4>> host_points = d.getFoundPoints();
        d.detectObstacles((int)rec.size(), rec.data());
        REQUIRE(d.getFoundPoints() == host_points && d.getObstacleCounter() == 2, 25);
        REQUIRE(slurp(dir + "/pcl_0000.ply") == slurp(dir + "/pcl_0001.ply"), 26);
        // no hit: no file, the counter stays
        std::vector<float> none(77, range.first);
        d.build(dmap, 0, 0, none.data());
        d.detectObstacles();
        REQUIRE(d.getFoundObstacles().empty() && d.getObstacleCounter() == 2, 27);
        REQUIRE(slurp(dir + "/pcl_0002.ply").empty(), 28);
        std::printf("cpu ok\n");
        if (!gpu) return 0;

        // build() on the device == Samplepoint::calculateSamplepointValue per point
        d.build(dmap, 0, 0);
        for (size_t i = 0; i < sp.size(); i++) {
            mvsv::Samplepoint s = sp[i];
            s.calculateSamplepointValue(dmap);
            REQUIRE(s.value == d.getSamplepointVec()[i].value, 30);
        }
        // the demo's loop: both detectors on every frame of one stream
        auto sgbm = mvsv::StereoSGBM::create(0, 64, 9, 8 * 81, 32 * 81);
        std::vector<uint8_t> L(320 * 96), R(320 * 96);
        REQUIRE(mvsv_synth_pair(0x5EED0000u + 90, 320, 96, 0, 64, L.data(), R.data()) == MVSV_OK, 31);
        mvsv::Mat Lm = mvsv::Mat::wrap(L.data(), 96, 320, mvsv::MAT_8UC1, 320);
        mvsv::Mat Rm = mvsv::Mat::wrap(R.data(), 96, 320, mvsv::MAT_8UC1, 320);
        Stereopair pair(Lm, Rm);
        mvsv::Rect roi_u, roi_b;
        mvsv::createDMapROIS(96, 320, 64, roi_u, roi_b);
        mvsv::Mat direct;
        sgbm->compute(Lm, Rm, direct);
        mvsv::Mat work = direct(roi_u);
        mvsv::SamplepointDetection a(dir + "/a"), b(dir + "/b");
        mvsv::MeanDisparityDetection m(dir);
        a.init(work, Q, 0.1f, 30.f);
        b.init(work, Q, 0.1f, 30.f);
        m.init(work, Q, 0.1f, 30.f);
        mvsv::DisparityStream st(*sgbm, 320, 96, 2, &roi_u);
        st.setBatch(2);
        st.enableSamplepoints(a, &roi_u);
        st.push(pair);
        bool threw = false;
        try {
            st.enableSamplepoints(a, &roi_u);  // a frame is pending
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        REQUIRE(threw, 32);
        st.push(pair);
        mvsv::SampleFrame fr;  // reused from frame to frame
        for (int f = 0; f < 2; f++) {
            st.frontSamples(fr);
            mvsv::Mat map;
            float means[81];
            st.pop(map, means);
            for (int y = 0; y < 96; y++) REQUIRE(std::memcmp(map.ptr<int16_t>(y), direct.ptr<int16_t>(y), 640) == 0, 33);
            mvsv::Mat w = map(roi_u);
            m.build(w, 0, mvsv::MeanDisparityDetection::MEAN_VALUE, means);
            a.build(w, 0, 0, fr.values.data());
            REQUIRE(fr.hits.size() == (size_t)fr.count, 40);  // no cap: every hit is held
            if (f == 0)
                a.detectObstacles((int)fr.hits.size(), fr.hits.data());
            else
                a.detectObstacles(fr);
            b.build(w, 0, 0);  // values on the device from the host map
            b.detectObstacles();
            REQUIRE(fr.values.size() == b.getSamplepointVec().size(), 34);
            for (size_t i = 0; i < fr.values.size(); i++) REQUIRE(fr.values[i] == b.getSamplepointVec()[i].value, 35);
            REQUIRE((size_t)fr.count == b.getFoundPoints().size() && fr.count > 0, 36);
            REQUIRE(a.getFoundPoints() == b.getFoundPoints(), 37);
            const std::string name = "/pcl_000" + std::to_string(f) + ".ply";
            REQUIRE(!slurp(dir + "/a" + name).empty() && slurp(dir + "/a" + name) == slurp(dir + "/b" + name), 38);
        }
        // max_hits below the count, into the frame that still holds every record of
        // the last one: count stays the total, hits holds the first 5 and nothing else
        const mvsv::SampleFrame full = fr;
        const std::vector<std::array<float, 4>> all_points = b.getFoundPoints();
        REQUIRE(full.count > 5, 41);
        st.enableSamplepoints(a, &roi_u, 5);
        st.push(pair);
        st.frontSamples(fr);
        {
            mvsv::Mat map;
            st.pop(map);
            REQUIRE(fr.count == full.count && fr.hits.size() == 5, 42);
            REQUIRE(std::memcmp(fr.hits.data(), full.hits.data(), 5 * sizeof(mvsv_sample_hit)) == 0, 43);
            mvsv::Mat w = map(roi_u);
            a.build(w, 0, 0, fr.values.data());
            a.detectObstacles(fr);
            REQUIRE(a.getFoundPoints().size() == 5 && a.getFoundObstacles().size() == 5, 44);
            for (int k = 0; k < 5; k++) REQUIRE(a.getFoundPoints()[k] == all_points[k], 45);
        }
        // a cap above the number of points is the number of points
        st.enableSamplepoints(a, &roi_u, 1 << 30);
        st.push(pair);
        st.frontSamples(fr);
        {
            mvsv::Mat map;
            st.pop(map);
            REQUIRE(fr.count == full.count && fr.hits.size() == full.hits.size(), 46);
            REQUIRE(std::memcmp(fr.hits.data(), full.hits.data(), full.hits.size() * sizeof(mvsv_sample_hit)) == 0, 47);
        }
        st.disableSamplepoints();
        st.push(pair);
        threw = false;
        try {
            st.frontSamples(fr);
        } catch (const mvsv::Error& e) {
            threw = e.code() == MVSV_E_INVALID_ARG;
        }
        mvsv::Mat map;
        st.pop(map);
        REQUIRE(threw && st.pending() == 0, 39);
        std::printf("gpu ok\n");
    } catch (const mvsv::Error& e) {
        std::printf("error: %s\n", e.what());
        return 1;
    }
    return 0;
}
