// sanitize_scan_filter.cpp -- filter_scans_cpu (plain host code: the whole rule of lcd_filter_scans) driven from a stand-alone program, for a
// host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_scan_filter.cpp rtabmap_amd/host/ScanFilter.cpp -o scan_filter_asan
//   ./scan_filter_asan
//
// Scans whose buffers end with their last row: empty and tiny scans, sizes around a workgroup's 256 rows, every step from 1 to beyond the
// scan, ranges on and off, rows that are not finite, huge coordinates whose squares overflow, one voxel and one voxel per row, leaves that
// overflow the grid, K from 1 to 32 on scans smaller and larger than K, radius mode from no neighbour to all, duplicates, collinear and flat
// clouds, capacities from 0 to beyond the result, and the refused arguments.  Every result is checked against what the rule promises whatever
// the numbers are; exit status 0 and "ok" when all hold.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "ScanFilter.h"

using rtabmap_amd::filter_scans_cpu;
using rtabmap_amd::ScanFilterParams;
using rtabmap_amd::ScanFilterResult;

namespace {

int failures = 0, cases = 0;

void expect(bool ok, const char* what) {
    if (!ok) { ++failures; std::fprintf(stderr, "FAILED: %s\n", what); }
}

bool quiet_nan(float v) { uint32_t b; std::memcpy(&b, &v, 4); return b == 0x7fc00000u; }

// what holds whatever the numbers are
void check(const std::vector<float>& scan, const ScanFilterParams& p, int64_t cap, bool deviceEntry) {
    ++cases;
    const std::vector<float> exact(scan);                             // a buffer that ends with the last row
    ScanFilterResult r;
    const int rc = filter_scans_cpu(exact.empty() ? nullptr : exact.data(), (int64_t)exact.size() / 3, p, cap, deviceEntry, r);
    if (rc != 0) { expect(rc == 1 || rc == 5, "a refusal is LCD_ERR_INVALID or LCD_ERR_UNSUPPORTED"); return; }
    const bool normals = p.normalK > 0 || p.normalRadius > 0.0f;
    expect(r.status >= 0 && r.status <= 4, "the status is an lcd_scan_status");
    expect((int64_t)r.xyz.size() == cap * 3 && (int64_t)r.normals.size() == (normals ? cap * 3 : 0), "the region's size");
    expect(r.count >= 0 && r.count <= cap && (r.status == 0) == (r.count > 0), "count and status agree");
    expect(r.stageCounts[0] >= r.stageCounts[1] && r.stageCounts[1] >= 0, "the stages shrink");
    expect(r.status != 0 || r.stageCounts[2] == r.count, "the final stage is the count");
    for (int64_t i = 0; i < cap * 3; ++i) {
        const bool in = i < (int64_t)r.count * 3;
        expect(in ? std::isfinite(r.xyz[(size_t)i]) : quiet_nan(r.xyz[(size_t)i]), "rows are finite, the rest of the region quiet NaNs");
        if (normals) expect(in ? std::isfinite(r.normals[(size_t)i]) : quiet_nan(r.normals[(size_t)i]), "normals are finite, the rest quiet NaNs");
    }
}

std::vector<float> cloud(int n, unsigned seed, float span) {
    std::mt19937 g(seed);
    std::uniform_real_distribution<float> u(-span, span);
    std::vector<float> x((size_t)n * 3);
    for (float& v : x) v = u(g);
    return x;
}

}  // namespace

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int sizes[] = {0, 1, 2, 3, 4, 5, 6, 31, 32, 33, 255, 256, 257, 513};
    for (int n : sizes) {
        const std::vector<float> s = cloud(n, 100u + (unsigned)n, 1.0f);
        for (int step : {0, 1, 2, 3, 256, 1000}) {
            ScanFilterParams p;
            p.downsamplingStep = step; p.rangeMin = 0.2f; p.rangeMax = 1.5f;
            check(s, p, n, false);
            p.is2d = true;
            check(s, p, n / 2, false);
        }
        for (float leaf : {1e-30f, 1e-6f, 0.01f, 0.3f, 10.0f, 1e30f}) {
            ScanFilterParams p;
            p.voxelSize = leaf;
            check(s, p, n, false);
        }
        for (int k = 1; k <= 32; ++k) {
            ScanFilterParams p;
            p.normalK = k; p.groundNormalsUp = k % 2 ? 0.8f : 0.0f; p.voxelSize = k % 3 ? 0.0f : 0.25f;
            check(s, p, n, false);
            check(s, p, n / 3, false);
        }
        for (float radius : {1e-20f, 0.05f, 0.5f, 10.0f, 3e19f, 3e38f}) {
            ScanFilterParams p;
            p.normalRadius = radius; p.viewpoint[2] = 3.0f;
            check(s, p, n, false);
        }
    }
    {   // rows that are not finite, coordinates whose squares and differences overflow
        std::vector<float> s = cloud(300, 7, 1.0f);
        s[0] = nan; s[3 * 255 + 1] = inf; s[3 * 256 + 2] = -inf;
        ScanFilterParams p;
        p.normalK = 5; p.voxelSize = 0.2f; p.rangeMax = 10.0f;
        check(s, p, 300, true);
        check(s, p, 300, false);
        std::vector<float> huge = cloud(64, 8, 3e38f);
        check(huge, p, 64, false);
        p.voxelSize = 0.0f;
        check(huge, p, 64, false);
        p.normalK = 0; p.normalRadius = 1e19f;
        check(huge, p, 64, false);
    }
    {   // duplicates, a line, a plane, one voxel, a lattice
        std::vector<float> dup, line, flat, lattice;
        for (int i = 0; i < 90; ++i) for (int c = 0; c < 3; ++c) dup.push_back((float)((i / 3) % 7) * (c + 1));
        for (int i = 0; i < 40; ++i) { line.push_back((float)i); line.push_back(2.0f * i); line.push_back(0.0f); }
        for (int i = 0; i < 64; ++i) { flat.push_back((float)(i % 8)); flat.push_back((float)(i / 8)); flat.push_back(0.0f); }
        for (int i = 0; i < 125; ++i) { lattice.push_back((float)(i % 5)); lattice.push_back((float)(i / 5 % 5)); lattice.push_back((float)(i / 25)); }
        for (const std::vector<float>* s : {&dup, &line, &flat, &lattice}) {
            ScanFilterParams p;
            p.normalK = 5;
            check(*s, p, 200, false);
            p.normalK = 0; p.normalRadius = 1.0f;
            check(*s, p, 200, false);
            p.voxelSize = 100.0f;
            check(*s, p, 1, false);
            check(*s, p, 0, false);
        }
    }
    {   // the refusals
        const std::vector<float> s = cloud(50, 9, 1.0f);
        ScanFilterResult r;
        ScanFilterParams p;
        auto refused = [&](const ScanFilterParams& q, int code, const char* what) { ++cases; expect(filter_scans_cpu(s.data(), 50, q, 50, false, r) == code, what); };
        p.normalK = 5; p.normalRadius = 0.3f; refused(p, 1, "K and radius together");
        p = ScanFilterParams(); p.normalK = 33; refused(p, 1, "K above 32");
        p = ScanFilterParams(); p.normalK = -1; refused(p, 1, "a negative K");
        p = ScanFilterParams(); p.voxelSize = -1.0f; refused(p, 1, "a negative leaf");
        p = ScanFilterParams(); p.voxelSize = nan; refused(p, 1, "a leaf that is no number");
        p = ScanFilterParams(); p.rangeMax = inf; refused(p, 1, "an infinite range");
        p = ScanFilterParams(); p.viewpoint[1] = nan; refused(p, 1, "a viewpoint that is no number");
        p = ScanFilterParams(); p.groundNormalsUp = -0.1f; refused(p, 1, "a negative ground threshold");
        p = ScanFilterParams(); p.normalK = 5; p.is2d = true; refused(p, 5, "2-D normals");
        const std::vector<float> big((size_t)16385 * 3, 0.5f);
        ++cases;
        expect(filter_scans_cpu(big.data(), 16385, ScanFilterParams(), 16385, false, r) == 5, "16385 sampled rows");
        p = ScanFilterParams(); p.downsamplingStep = 2;
        check(big, p, 8192, false);
    }
    if (failures) { std::fprintf(stderr, "%d of %d cases failed\n", failures, cases); return 1; }
    std::printf("ok: %d cases\n", cases);
    return 0;
}
