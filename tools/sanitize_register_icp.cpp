// sanitize_register_icp.cpp -- register_icp_cpu (plain host code: the whole rule of lcd_register_icp) driven from a stand-alone program, for a
// host-only AddressSanitizer / UndefinedBehaviorSanitizer run.  No engine is created and nothing touches a GPU.
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Irtabmap_amd/host \
//       tools/sanitize_register_icp.cpp rtabmap_amd/host/RegistrationIcp.cpp -o register_icp_asan
//   ./register_icp_asan
//
// Scans whose buffers end with their last row (a read past a scan is a heap overflow): empty and tiny clouds, sides around a workgroup's 256
// rows, clouds that are all one point, rows that are not finite (refused by the host entry's rules, left out by the device entry's), huge
// coordinates whose distances and sums overflow (and lie beyond the grid's cell range), thresholds tiny and huge, both estimators, every
// stop, 8192 rows, and the refused arguments.
// Every case runs in the brute and in the grid form of the search, which must agree to the bit, and every result is checked against what the
// rule promises whatever the numbers are; exit status 0 and "ok" when all hold.
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

using rtabmap_amd::IcpResult;
using rtabmap_amd::register_icp_cpu;

namespace {

typedef std::vector<float> Scan;                                       // [n x 3]
const float IDENTITY[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};

int failures = 0;
void expect(bool ok, const char* what, int tag) {
    if (!ok) { std::printf("FAILED: %s (case %d)\n", what, tag); ++failures; }
}

struct Params {
    int iterations = 10, laser = 0;
    bool flat = false, device = false;
    double dist = 0.3;
    float epsilon = 0.0f, ratio = 0.1f;
    const float* guess = IDENTITY;
};

// heap copies that end with the last element
bool run(const Scan& f, const Scan& t, const Params& p, IcpResult& r) {
    Scan fx(f), tx(t);
    fx.shrink_to_fit(); tx.shrink_to_fit();
    std::vector<float> g(p.guess, p.guess + 12);
    g.shrink_to_fit();
    return register_icp_cpu(fx.data(), (int)f.size() / 3, tx.data(), (int)t.size() / 3, g.data(), p.iterations, p.flat, p.laser, p.dist, p.epsilon, p.ratio, 0,
                            p.device, r);
}
bool run_grid(const Scan& f, const Scan& t, const Params& p, IcpResult& r) {
    Scan fx(f), tx(t);
    fx.shrink_to_fit(); tx.shrink_to_fit();
    return register_icp_cpu(fx.data(), (int)f.size() / 3, tx.data(), (int)t.size() / 3, p.guess, p.iterations, p.flat, p.laser, p.dist, p.epsilon, p.ratio, 2, p.device, r);
}

bool all_zero(const float* t) { for (int k = 0; k < 12; ++k) if (t[k] != 0.0f) return false; return true; }
bool row_finite(const Scan& s, int i) { return std::isfinite(s[3 * i]) && std::isfinite(s[3 * i + 1]) && std::isfinite(s[3 * i + 2]); }

void check(const Scan& f, const Scan& t, const Params& p, int tag) {
    IcpResult a, b;
    expect(run(f, t, p, a), "accepted", tag);
    expect(run_grid(f, t, p, b), "accepted in the grid form", tag);
    expect(std::memcmp(a.transform, b.transform, 48) == 0 && std::memcmp(a.icpTransform, b.icpTransform, 48) == 0 && std::memcmp(a.correction, b.correction, 48) == 0 &&
           a.status == b.status && a.stop == b.stop && a.iterations == b.iterations && a.correspondences == b.correspondences && a.match == b.match &&
           std::memcmp(&a.variance, &b.variance, 8) == 0 && std::memcmp(&a.ratio, &b.ratio, 4) == 0, "the grid form gives the brute form's bits", tag);
    const int nf = (int)f.size() / 3, nt = (int)t.size() / 3;
    int pf = 0, pt = 0;
    for (int i = 0; i < nf; ++i) pf += row_finite(f, i);
    for (int j = 0; j < nt; ++j) pt += row_finite(t, j);
    expect((int)a.match.size() == nf, "one match entry per from-row", tag);
    expect(a.status >= 0 && a.status <= 3 && a.stop >= 0 && a.stop <= 4, "a status and a stop of the enums", tag);
    expect((a.status == 1) == (pf == 0 || pt == 0), "LCD_ICP_EMPTY iff a side has no participating row", tag);
    expect(a.iterations >= 0 && a.iterations <= p.iterations, "iterations within max_iterations", tag);
    expect((a.status == 2) == (a.stop == 4) && (a.status == 1) == (a.stop == 0), "the stop goes with the status", tag);
    if (a.stop == 1) expect(a.iterations == p.iterations, "the iterations stop at max_iterations", tag);
    if (a.status != 0) expect(all_zero(a.transform), "no transform without LCD_ICP_OK", tag);
    if (a.status == 1 || a.status == 2)
        expect(all_zero(a.icpTransform) && all_zero(a.correction) && a.correspondences == 0 && a.ratio == 0.0f && a.variance == 1.0, "nothing without convergence", tag);
    std::set<int> used;
    int kept = 0;
    for (int i = 0; i < nf; ++i) {
        const int j = a.match[(size_t)i];
        if (j < 0) { expect(j == -1, "no match is -1", tag); continue; }
        ++kept;
        expect(j < nt && row_finite(f, i) && row_finite(t, j) && used.insert(j).second, "a match joins two participating rows, each to-row once", tag);
    }
    expect(kept == a.correspondences && kept <= std::min(pf, pt), "out_match holds the correspondences", tag);
    if (a.status == 0 || a.status == 3) {
        const float want = (float)kept / (float)(p.laser > 0 ? p.laser : std::max(pf, pt));
        expect(std::memcmp(&want, &a.ratio, 4) == 0, "the ratio", tag);
        expect((a.status == 3) == (a.ratio <= p.ratio), "the ratio gate", tag);
        expect(kept >= 3 ? (a.variance >= 0.0 || std::isnan(a.variance)) : a.variance == 1.0, "a variance from three correspondences on", tag);
    }
}

Scan cloud(int n, std::mt19937& rng, bool flat) {
    std::uniform_real_distribution<float> u(-3.0f, 3.0f);
    Scan s;
    for (int i = 0; i < n; ++i) { s.push_back(u(rng)); s.push_back(u(rng)); s.push_back(flat ? 0.0f : u(rng)); }
    return s;
}

// a small turn about z and a shift, with noise
Scan moved(const Scan& f, std::mt19937& rng, float noise, bool flat) {
    std::normal_distribution<float> g(0.0f, noise);
    Scan t;
    for (size_t i = 0; i < f.size(); i += 3) {
        t.push_back(0.9995f * f[i] - 0.0316f * f[i + 1] + 0.05f + g(rng));
        t.push_back(0.0316f * f[i] + 0.9995f * f[i + 1] - 0.03f + g(rng));
        t.push_back(flat ? 0.0f : f[i + 2] + 0.02f + g(rng));
    }
    return t;
}

}  // namespace

int main() {
    std::mt19937 rng(7);
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    int tag = 0;

    // empty and tiny clouds, sides around a workgroup, both estimators, sizes that differ either way (the target swap)
    for (bool flat : {false, true})
        for (int nf : {0, 1, 2, 3, 4, 255, 256, 257, 513})
            for (int nt : {0, 1, 2, 3, 256, 300}) {
                const Scan f = cloud(nf, rng, flat), base = cloud(nt, rng, flat);
                Scan t = nt && nf ? moved(Scan(f.begin(), f.begin() + 3 * std::min(nf, nt)), rng, 0.003f, flat) : base;
                t.insert(t.end(), base.begin() + (long)t.size(), base.end());
                Params p;
                p.flat = flat;
                check(f, t, p, ++tag);
                p.laser = 100; p.ratio = 0.5f; p.epsilon = 1e-3f;
                check(f, t, p, ++tag);
            }
    // every stop: one iteration, an epsilon that ends it early, identical clouds
    {
        const Scan f = cloud(200, rng, false), t = moved(f, rng, 0.002f, false);
        Params p;
        p.iterations = 1; check(f, t, p, ++tag);
        p.iterations = 50; p.epsilon = 0.01f; check(f, t, p, ++tag);
        p.epsilon = 0.0f; check(f, f, p, ++tag);
        IcpResult r;
        expect(run(f, f, p, r) && r.status == 0 && r.correspondences == 200 && r.variance == 0.0 && std::memcmp(r.icpTransform, IDENTITY, 48) == 0,
               "identical clouds: the identity, exactly", tag);
    }
    // clouds that are one point many times (every sum of products is zero), ties everywhere
    for (bool flat : {false, true}) {
        Scan one;
        for (int i = 0; i < 40; ++i) { one.push_back(1.0f); one.push_back(-2.0f); one.push_back(flat ? 0.0f : 0.5f); }
        Scan other(one);
        for (size_t i = 0; i < other.size(); i += 3) other[i] += 0.125f;
        Params p;
        p.flat = flat;
        check(one, other, p, ++tag);
        check(one, one, p, ++tag);
    }
    // rows that are not finite: left out under the device entry's rules, refused under the host entry's
    {
        Scan f = cloud(600, rng, false), t = moved(f, rng, 0.003f, false);
        for (int r : {0, 255, 256, 511, 599}) { f[3 * r + r % 3] = r % 2 ? nan : inf; t[3 * r + (r + 1) % 3] = r % 2 ? -inf : nan; }
        Params p;
        p.device = true;
        check(f, t, p, ++tag);
        IcpResult r;
        r.status = -9;
        p.device = false;
        expect(!run(f, t, p, r) && r.status == -9, "the host entry refuses a row that is not finite", tag);
        Scan bad(30, nan);
        p.device = true;
        check(bad, t, p, ++tag);
        check(f, bad, p, ++tag);
    }
    // huge coordinates: distances, sums and the guess's products overflow
    for (float scale : {1.0e15f, 4.4e18f, 1.0e19f, 3.0e38f}) {
        Scan f = cloud(64, rng, false);
        for (float& v : f) v *= scale / 3.0f;
        const Scan t = moved(f, rng, 0.0f, false);
        const float turn[12] = {0, -1, 0, scale, 1, 0, 0, -scale, 0, 0, 1, 0};
        for (double d : {0.1, 1.0e15, 1.0e150}) {
            Params p;
            p.dist = d;
            check(f, t, p, ++tag);
            p.flat = true; p.guess = turn;
            check(f, t, p, ++tag);
        }
    }
    // denormal coordinates and a tiny threshold
    {
        Scan f = cloud(30, rng, false);
        for (float& v : f) v *= 1.0e-42f;
        Params p;
        check(f, f, p, ++tag);
        p.dist = 1.0e-40;
        check(f, moved(f, rng, 1.0e-44f, false), p, ++tag);
    }
    // the largest scans
    {
        const Scan f = cloud(8192, rng, false), t = moved(f, rng, 0.002f, false);
        Params p;
        p.iterations = 2;
        check(f, t, p, ++tag);
    }
    // refused arguments leave the result alone
    {
        const Scan f = cloud(5, rng, false);
        IcpResult r;
        r.status = -9;
        auto refused = [&](void (*change)(Params&)) { Params p; change(p); return !run(f, f, p, r); };
        expect(refused([](Params& p) { p.iterations = 0; }) && refused([](Params& p) { p.laser = -1; }) && refused([](Params& p) { p.dist = 0.0; }) &&
               refused([](Params& p) { p.dist = -1.0; }) && refused([](Params& p) { p.dist = std::numeric_limits<double>::quiet_NaN(); }) &&
               refused([](Params& p) { p.dist = std::numeric_limits<double>::infinity(); }) && refused([](Params& p) { p.dist = 1.0e200; }) &&
               refused([](Params& p) { p.epsilon = -1.0f; }) && refused([](Params& p) { p.epsilon = std::numeric_limits<float>::quiet_NaN(); }) &&
               refused([](Params& p) { p.ratio = 1.5f; }) && refused([](Params& p) { p.ratio = -0.5f; }), "refused", ++tag);
        const float bad_guess[12] = {1, 0, 0, nan, 0, 1, 0, 0, 0, 0, 1, 0};
        Params p;
        p.guess = bad_guess;
        expect(!run(f, f, p, r), "a guess that is not finite", tag);
        expect(!run(cloud(8193, rng, false), f, Params(), r) && !run(f, cloud(8193, rng, false), Params(), r) && r.status == -9, "more than 8192 rows", tag);
        expect(!register_icp_cpu(nullptr, 5, f.data(), 5, IDENTITY, 10, false, 0, 0.3, 0.0f, 0.1f, 0, false, r), "a null scan", tag);
        expect(!register_icp_cpu(f.data(), 5, f.data(), 5, nullptr, 10, false, 0, 0.3, 0.0f, 0.1f, 0, false, r), "a null guess", tag);
        expect(!register_icp_cpu(f.data(), 5, f.data(), 5, IDENTITY, 10, false, 0, 0.3, 0.0f, 0.1f, 7, false, r) && r.status == -9, "no search", tag);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("ok: %d cases\n", tag);
    return 0;
}
