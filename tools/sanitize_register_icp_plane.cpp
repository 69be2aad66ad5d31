// sanitize_register_icp_plane.cpp -- register_icp_plane_cpu (plain host code: the whole rule of lcd_register_icp_plane) driven from a stand-alone
// program, for a host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_register_icp_plane.cpp rtabmap_amd/host/RegistrationIcp.cpp -o register_icp_plane_asan
//   ./register_icp_plane_asan
//
// Scans and normals whose buffers end with their last row: empty and tiny clouds (fewer rows than the fit's six unknowns), sides around a
// workgroup's 256 rows, room-like and corridor-like normals, every normal the same, one and two finite normals a side, normals and
// coordinates that are not finite, zero normals, huge coordinates and normals whose sums overflow, the three strategies, the gate at every
// cosine from -1 to 1, both estimators of the fallback, force_3dof, 8192 rows, and the refused arguments.  Every case runs in the brute and
// in the grid form of the search, which must agree to the bit, and every result is checked against what the rule promises whatever the
// numbers are; exit status 0 and "ok" when all hold.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <set>
#include <vector>

#include "RegistrationIcp.h"

// RegistrationIcp.cpp's engine entries are linked but never called here
struct lcd_icp_args;
struct lcd_icp_plane_args;
struct lcd_scan_filter_args;
extern "C" int lcd_register_icp(lcd_engine*, const lcd_icp_args*) { return 1; }
extern "C" int lcd_register_icp_plane(lcd_engine*, const lcd_icp_plane_args*) { return 1; }
extern "C" int lcd_filter_scans(lcd_engine*, const lcd_scan_filter_args*) { return 1; }

using rtabmap_amd::IcpPlaneResult;
using rtabmap_amd::register_icp_plane_cpu;

namespace {

typedef std::vector<float> Rows;                                       // [n x 3]
const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
const float TILTED[12] = {0.9992f, -0.0399f, 0.0f, 0.05f, 0.0399f, 0.9992f, 0.0f, -0.03f, 0.0f, 0.0f, 1.0f, 0.02f};

int failures = 0, cases = 0;
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

struct Params {
    int iterations = 10, laser = 0, strategy = 1;
    bool flat = false, device = false, gate = false;
    double dist = 0.3, cosine = 0.7;
    float epsilon = 0.0f, ratio = 0.1f, complexity = 0.02f;
    const float* guess = IDENTITY;
};

struct Scan { Rows xyz, normals; int n() const { return (int)xyz.size() / 3; } };

// heap copies that end with the last element
bool run(const Scan& f, const Scan& t, const Params& p, int search, IcpPlaneResult& r) {
    Rows fx(f.xyz), fn(f.normals), tx(t.xyz), tn(t.normals);
    fx.shrink_to_fit(); fn.shrink_to_fit(); tx.shrink_to_fit(); tn.shrink_to_fit();
    std::vector<float> g(p.guess, p.guess + 12);
    g.shrink_to_fit();
    return register_icp_plane_cpu(fx.data(), fn.data(), f.n(), tx.data(), tn.data(), t.n(), g.data(), p.iterations, p.flat, p.laser, p.dist, p.epsilon, p.ratio,
                                  p.complexity, p.strategy, p.gate, p.cosine, search, p.device, r);
}

bool all_zero(const float* t, int n = 12) { for (int k = 0; k < n; ++k) if (t[k] != 0.0f) return false; return true; }
bool row_finite(const Rows& s, int i) { return std::isfinite(s[3 * i]) && std::isfinite(s[3 * i + 1]) && std::isfinite(s[3 * i + 2]); }

void check(const Scan& f, const Scan& t, const Params& p, int tag) {
    ++cases;
    IcpPlaneResult a, b;
    expect(run(f, t, p, 1, a), "accepted", tag);
    expect(run(f, t, p, 2, b), "accepted in the grid form", tag);
    expect(std::memcmp(a.transform, b.transform, 48) == 0 && std::memcmp(a.icpTransform, b.icpTransform, 48) == 0 && std::memcmp(a.correction, b.correction, 48) == 0 &&
           a.status == b.status && a.stop == b.stop && a.iterations == b.iterations && a.correspondences == b.correspondences && a.match == b.match &&
           std::memcmp(&a.variance, &b.variance, 8) == 0 && std::memcmp(&a.ratio, &b.ratio, 4) == 0 && a.branch == b.branch &&
           std::memcmp(&a.complexity, &b.complexity, 4) == 0 && std::memcmp(a.complexityVectors, b.complexityVectors, 36) == 0, "the grid form gives the brute form's bits", tag);
    const int nf = f.n(), nt = t.n();
    int rows_f = 0, rows_t = 0, part_f = 0, part_t = 0, oi_f = 0, oi_t = 0;
    for (int i = 0; i < nf; ++i) { rows_f += row_finite(f.xyz, i); oi_f += row_finite(f.normals, i); part_f += row_finite(f.xyz, i) && row_finite(f.normals, i); }
    for (int j = 0; j < nt; ++j) { rows_t += row_finite(t.xyz, j); oi_t += row_finite(t.normals, j); part_t += row_finite(t.xyz, j) && row_finite(t.normals, j); }
    expect((int)a.match.size() == nf, "one match entry per from-row", tag);
    expect(a.status >= 0 && a.status <= 4 && a.stop >= 0 && a.stop <= 5 && (a.branch == 0 || a.branch == 1), "a status, a stop and a branch of the enums", tag);
    if (oi_f <= 1 || oi_t <= 1) expect(a.complexity == 0.0f && all_zero(a.complexityValues, 3) && all_zero(a.complexityVectors, 9), "no PCA with a side of one normal", tag);
    expect((a.status == 4) == (p.strategy == 0 && a.complexity < p.complexity), "LCD_ICP_LOW_COMPLEXITY iff strategy 0 meets a low complexity", tag);
    if (a.status != 4) {
        expect((a.branch == 1) == (a.complexity < p.complexity), "branch 1 iff the complexity is below min_complexity", tag);
        const int mf = a.branch == 0 ? part_f : rows_f, mt = a.branch == 0 ? part_t : rows_t;
        expect((a.status == 1) == (mf == 0 || mt == 0), "LCD_ICP_EMPTY iff a side has no participating row", tag);
    } else {
        expect(a.branch == 0 && a.iterations == 0 && a.stop == 0, "nothing ran with LCD_ICP_LOW_COMPLEXITY", tag);
    }
    if (!(a.complexity < p.complexity && a.complexity > 0.0f)) expect(a.secondEigenvalue == 1.0f, "the second value is 1 off the low-complexity path with vectors", tag);
    expect(a.iterations >= 0 && a.iterations <= p.iterations, "iterations within max_iterations", tag);
    expect((a.status == 2) == (a.stop == 4 || a.stop == 5), "the stop goes with the status", tag);
    if (a.stop == 5) expect(a.branch == 0, "only the point-to-plane system is singular", tag);
    if (a.stop == 1) expect(a.iterations == p.iterations, "the iterations stop at max_iterations", tag);
    if (a.status != 0) expect(all_zero(a.transform), "no transform without LCD_ICP_OK", tag);
    if (a.status == 1 || a.status == 2 || a.status == 4)
        expect(all_zero(a.icpTransform) && all_zero(a.correction) && a.correspondences == 0 && a.ratio == 0.0f && a.variance == 1.0, "nothing without convergence", tag);
    std::set<int> used;
    int kept = 0;
    for (int i = 0; i < nf; ++i) {
        const int j = a.match[(size_t)i];
        expect(j >= -1 && j < nt, "a match inside the to-region", tag);
        if (j < 0) continue;
        ++kept;
        expect(row_finite(f.xyz, i) && row_finite(t.xyz, j), "only rows with finite coordinates are matched", tag);
        if (a.branch == 0) expect(row_finite(f.normals, i) && row_finite(t.normals, j), "branch 0 matches only rows with a finite normal", tag);
        expect(used.insert(j).second, "a to-row is matched once", tag);
    }
    expect(kept == a.correspondences, "out_match lists the correspondences counted", tag);
    if (a.status == 0 || a.status == 3) {
        const int den = p.laser > 0 ? p.laser : std::max(rows_f, rows_t);
        expect(a.ratio == (float)a.correspondences / (float)den, "the ratio's denominator counts rows with finite coordinates", tag);
        expect((a.status == 3) == (a.ratio <= p.ratio), "the ratio gate", tag);
        if (a.branch == 0) expect((a.variance == 1.0) == (a.correspondences == 0) || a.variance == 1.0, "branch 0 takes a variance from one correspondence on", tag);
        else if (a.correspondences < 3) expect(a.variance == 1.0, "branch 1 keeps the >= 3 guard", tag);
        if (a.branch == 0 && p.flat) expect(a.icpTransform[2] == 0.0f && a.icpTransform[6] == 0.0f && a.icpTransform[10] == 1.0f && a.icpTransform[11] == 0.0f, "to3DoF", tag);
    }
}

Scan room(std::mt19937& rng, int n, float noise, bool corridor = false) {
    std::uniform_real_distribution<float> u(0.0f, 4.0f), v(0.0f, 3.0f);
    std::normal_distribution<float> g(0.0f, 1.0f);
    Scan s;
    for (int i = 0; i < n; ++i) {
        const int which = corridor ? (int)(rng() % 16 == 0) + (int)(rng() % 64 == 0) : (int)(rng() % 3);
        const float a = u(rng), b = v(rng);
        const float p[3][3] = {{a, b, 0.0f}, {a, 0.0f, b}, {0.0f, a, b}}, nrm[3][3] = {{0, 0, 1}, {0, 1, 0}, {1, 0, 0}};
        for (int k = 0; k < 3; ++k) { s.xyz.push_back(p[which][k] + noise * g(rng)); s.normals.push_back(nrm[which][k]); }
    }
    return s;
}
Scan moved(const Scan& s, float dx, float dy, float dz) {
    Scan o(s);
    for (int i = 0; i < o.n(); ++i) { o.xyz[3 * i] += dx; o.xyz[3 * i + 1] += dy; o.xyz[3 * i + 2] += dz; }
    return o;
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int tag = 0;
    const int sizes[] = {0, 1, 2, 3, 5, 6, 7, 255, 256, 257, 511, 513};
    for (int nf : sizes)
        for (int nt : {0, 1, 5, 6, 7, 256, 300}) {
            const Scan f = room(rng, nf, 0.004f), t = moved(room(rng, nt, 0.004f), 0.03f, -0.02f, 0.01f);
            Params p;
            check(f, t, p, ++tag);
            p.flat = true; p.gate = true;
            check(f, t, p, ++tag);
        }
    // the strategies, the gate's cosines, both branches with and without force_3dof, a guess
    for (bool corridor : {false, true})
        for (int strategy : {0, 1, 2})
            for (double cosine : {-1.0, 0.0, 0.7, 1.0, 2.0}) {
                const Scan f = room(rng, 300, 0.004f, corridor), t = moved(room(rng, 280, 0.004f, corridor), 0.03f, -0.02f, 0.01f);
                Params p;
                p.strategy = strategy; p.gate = true; p.cosine = cosine; p.guess = TILTED; p.iterations = 6;
                check(f, t, p, ++tag);
                p.flat = true; p.laser = 500; p.complexity = corridor ? 0.5f : 0.0f;
                check(f, t, p, ++tag);
            }
    // normals: all the same, one and two finite a side, NaN and infinite, zero, huge; coordinates that are not finite on the device entry
    {
        Scan f = room(rng, 300, 0.004f), t = moved(room(rng, 300, 0.004f), 0.02f, 0.0f, 0.0f);
        Scan same_f(f), same_t(t);
        for (int i = 0; i < 300; ++i) for (int k = 0; k < 3; ++k) { same_f.normals[3 * i + k] = k == 1; same_t.normals[3 * i + k] = k == 1; }
        for (float c : {0.0f, 0.02f, 1.0f})
            for (int strategy : {0, 1, 2}) { Params p; p.complexity = c; p.strategy = strategy; check(same_f, same_t, p, ++tag); }
        for (int keep : {0, 1, 2, 3}) {
            Scan a(f), b(t);
            for (int i = keep; i < 300; ++i) { a.normals[3 * i] = nan; b.normals[3 * i + 2] = i % 2 ? inf : -inf; }
            Params p;
            check(a, b, p, ++tag);
            p.complexity = 0.0f;
            check(a, b, p, ++tag);
        }
        Scan z(f), h(t);
        for (int i = 0; i < 300; i += 3) { z.normals[3 * i] = z.normals[3 * i + 1] = z.normals[3 * i + 2] = 0.0f; h.normals[3 * i + 1] = 3e38f; }
        Params p;
        p.gate = true;
        check(z, h, p, ++tag);
        p.complexity = 0.0f;
        check(z, h, p, ++tag);
        Scan bad(f);
        bad.xyz[3 * 255] = nan; bad.xyz[3 * 256 + 1] = inf; bad.normals[3 * 257 + 2] = nan;
        IcpPlaneResult r;
        ++cases;
        expect(!run(bad, t, p, 1, r), "the host entry refuses a coordinate that is not finite", ++tag);
        p.device = true;
        check(bad, t, p, ++tag);
        Scan huge(f);
        huge.xyz[0] = 3e38f; huge.xyz[4] = -3e38f; huge.xyz[8] = 1e30f;
        p.dist = 1e10;
        check(huge, t, p, ++tag);
    }
    // 8192 rows
    {
        Params p;
        p.iterations = 2; p.gate = true;
        check(room(rng, 8192, 0.003f), moved(room(rng, 8192, 0.003f), 0.02f, 0.01f, 0.0f), p, ++tag);
    }
    // the refused arguments
    {
        const Scan f = room(rng, 20, 0.0f), t = room(rng, 20, 0.0f);
        IcpPlaneResult r;
        auto refused = [&](Params p, int search, const char* what) { ++cases; expect(!run(f, t, p, search, r), what, ++tag); };
        Params p;
        p.iterations = 0; refused(p, 0, "max_iterations < 1");
        p = Params(); p.laser = -1; refused(p, 0, "max_laser_scans < 0");
        p = Params(); refused(p, 3, "a search that is none");
        p = Params(); p.dist = 0.0; refused(p, 0, "a distance of 0");
        p = Params(); p.dist = 1e200; refused(p, 0, "a distance whose square is not finite");
        p = Params(); p.epsilon = nan; refused(p, 0, "an epsilon that is not finite");
        p = Params(); p.ratio = 1.5f; refused(p, 0, "a ratio above 1");
        p = Params(); p.complexity = -0.1f; refused(p, 0, "a negative min_complexity");
        p = Params(); p.complexity = 1.5f; refused(p, 0, "a min_complexity above 1");
        p = Params(); p.complexity = nan; refused(p, 0, "a min_complexity that is not a number");
        p = Params(); p.strategy = 3; refused(p, 0, "a strategy above 2");
        p = Params(); p.strategy = -1; refused(p, 0, "a negative strategy");
        p = Params(); p.gate = true; p.cosine = nan; refused(p, 0, "a cosine that is not finite while the gate is on");
        p = Params(); p.cosine = nan; ++cases; expect(run(f, t, p, 0, r), "a cosine that is not finite is legal while the gate is off", ++tag);
        ++cases;
        expect(!register_icp_plane_cpu(f.xyz.data(), nullptr, 20, t.xyz.data(), t.normals.data(), 20, IDENTITY, 10, false, 0, 0.3, 0.0f, 0.1f, 0.02f, 1, false, 0.0, 0, false, r),
               "null normals where rows exist", ++tag);
    }
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ok: %d cases\n", cases);
    return 0;
}
