// Driver for the decision behind ecc_metric_set_form_incremental (epipolarconsistency_amd/csrc/ecc_form_base.h) and for the position
// rule its copy kernel scatters by (csrc/ecc_pose_scatter.h), CPU only: its own main, no HIP, no library.
//   decide      nothing kept -> MISS; identical matrices -> HIT; one, two and limit(n) changed views (views 0 and n - 1 among them, a
//               difference in the sign of a zero or in the last bit) -> REFRESH with exactly those views, ascending; limit + 1 -> MISS;
//               each single key field changed -> MISS; the caller's radius rule refusing -> MISS; ECC_SAMPLING_REFERENCE -> MISS
//               and may_keep() false; a smaller caller's bound is kept to
//   limit       min(ECC_POSE_BATCH_MAX_MOVED, n / 4); base_pairs: n (n - 1) / 2, 0, c (n - 1) - c (c - 1) / 2
//   position    for n = 12 (and 2, 5, 40) and the changed sets {0}, {n - 1}, {0, n - 1}, {3, 4, 5}, ...: the non-hole entries (u, a) of
//               the c-column grid map ONE-TO-ONE onto exactly the pairs that contain a changed view, and their number is base_pairs
// Built by tests/test_form_incremental_abi.py with -Wall -Werror -fsanitize=address,undefined and run directly.
#include <cmath>
#include <cstdio>
#include <set>

#include "../../epipolarconsistency_amd/csrc/ecc_form_base.h"
#include "../../epipolarconsistency_amd/csrc/ecc_pose_scatter.h"

namespace fb = ecc_form_base;

namespace {

int failures = 0;
void check(bool ok, const char* what, long long a = 0, long long b = 0)
{
    if (ok) return;
    if (++failures <= 20) std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
}

fb::Key a_key(int n)
{
    fb::Key k;
    k.kind = fb::VARIANCE_ROBUST;
    k.T = 4;
    k.S = 3;
    k.loss = 1;
    k.delta = fb::bits_of(2.5f);
    k.floor = fb::bits_of(1.5f);
    k.mode = ECC_SAMPLING_POLYNOMIAL;
    k.radius = fb::bits_of(120.f);
    k.dkappa = fb::bits_of(0.f);
    k.tol = fb::bits_of(0.02f);
    k.use_corr = 0;
    k.n_views = n;
    k.n_dtrs = 2 * n;
    return k;
}

std::vector<double> matrices(int n)
{
    std::vector<double> P(12 * (size_t)n);
    for (size_t k = 0; k < P.size(); ++k) P[k] = (double)(k % 89) - 44.0;  // zeros included
    return P;
}

// a difference in the bits only: the sign of a zero, or the last bit
void touch(std::vector<double>& P, int v, int q)
{
    double& x = P[12 * (size_t)v + q];
    x = x == 0.0 ? -0.0 : std::nextafter(x, 1e300);
}

const auto keeps = [](const std::vector<int>&) { return true; };

void check_decide(int n)
{
    const fb::Key key = a_key(n);
    const std::vector<double> kept = matrices(n);
    const int64_t lim = fb::limit(n);
    check(lim == std::min<int64_t>(32, n / 4), "limit", n, lim);
    std::vector<int> changed;
    check(fb::decide(false, key, kept.data(), key, kept.data(), lim, keeps, &changed) == fb::MISS, "nothing kept", n);
    check(fb::decide(true, key, nullptr, key, kept.data(), lim, keeps, &changed) == fb::MISS, "no kept matrices", n);
    check(fb::decide(true, key, kept.data(), key, kept.data(), lim, keeps, &changed) == fb::HIT && changed.empty(), "identical", n);
    // changed sets: one view (first, last, middle), two, the limit's number, one more
    std::vector<std::vector<int>> sets = {{0}, {n - 1}, {n / 2}, {0, n - 1}, {n / 3, n / 3 + 1}};
    for (int64_t c : {lim, lim + 1}) {
        std::vector<int> s;
        for (int64_t a = 0; a < c && a < n; ++a) s.push_back((int)(a * n / c));  // spread, ascending, view 0 among them
        sets.push_back(s);
        std::vector<int> top;
        for (int64_t a = 0; a < c && a < n; ++a) top.push_back((int)(n - c + a));  // the last c views
        if (c <= n) sets.push_back(top);
    }
    for (const auto& s : sets) {
        std::set<int> uniq(s.begin(), s.end());
        if (uniq.size() != s.size() || s.empty()) continue;
        std::vector<double> cur = kept;
        int q = 0;
        for (int v : s) touch(cur, v, (q += 5) % 12);
        const fb::Decision d = fb::decide(true, key, kept.data(), key, cur.data(), lim, keeps, &changed);
        if ((int64_t)s.size() <= lim) {
            check(d == fb::REFRESH && changed == s, "refresh lists exactly the changed views", n, (long long)s.size());
            check(fb::decide(true, key, kept.data(), key, cur.data(), lim, [](const std::vector<int>&) { return false; }, &changed) == fb::MISS,
                  "the radius rule refuses", n, (long long)s.size());
            if (s.size() > 1)
                check(fb::decide(true, key, kept.data(), key, cur.data(), (int64_t)s.size() - 1, keeps, &changed) == fb::MISS,
                      "a smaller bound of the caller's", n, (long long)s.size());
        } else {
            check(d == fb::MISS, "more than the limit", n, (long long)s.size());
        }
    }
    // each single key field
    std::vector<fb::Key> others(13, key);
    others[0].kind = fb::ROBUST;
    others[1].T = 3;
    others[2].S = 2;
    others[3].loss = 0;
    others[4].delta = fb::bits_of(std::nextafterf(2.5f, 3.f));
    others[5].floor = fb::bits_of(0.125f);
    others[6].mode = ECC_SAMPLING_PER_SAMPLE;
    others[7].radius = fb::bits_of(std::nextafterf(120.f, 121.f));
    others[8].dkappa = fb::bits_of(0.001f);
    others[9].tol = fb::bits_of(0.f);
    others[10].use_corr = 1;
    others[11].n_views = n + 1;
    others[12].n_dtrs = n;
    for (size_t f = 0; f < others.size(); ++f) {
        check(!(others[f] == key), "key field compared", (long long)f);
        if (f == 11) continue;  // (the kept matrices would be too few to compare: the key stops it before they are read -- below)
        check(fb::decide(true, key, kept.data(), others[f], kept.data(), lim, keeps, &changed) == fb::MISS, "a changed key field", n, (long long)f);
    }
    {
        const std::vector<double> more = matrices(n + 1);
        check(fb::decide(true, key, kept.data(), others[11], more.data(), lim, keeps, &changed) == fb::MISS, "another n_views", n);
    }
    // zero bits of a float parameter: -0.0f is another key than 0.0f
    fb::Key z = key, mz = key;
    z.dkappa = fb::bits_of(0.f);
    mz.dkappa = fb::bits_of(-0.f);
    check(!(z == mz), "floats bitwise");
    // the reference arithmetic: a miss although everything agrees, and nothing may be kept
    fb::Key ref = key;
    ref.mode = ECC_SAMPLING_REFERENCE;
    check(fb::decide(true, ref, kept.data(), ref, kept.data(), lim, keeps, &changed) == fb::MISS, "reference is a miss", n);
    check(!fb::may_keep(ref) && fb::may_keep(key) && !fb::may_keep(fb::Key()), "may_keep");
    check(fb::base_pairs(fb::MISS, n, 3) == (int64_t)n * (n - 1) / 2 && fb::base_pairs(fb::HIT, n, 3) == 0, "base_pairs", n);
}

void check_positions(int n, const std::vector<int>& M)
{
    const int c = (int)M.size();
    std::set<long long> got;
    long long entries = 0;
    for (int u = 0; u < n; ++u)
        for (int a = 0; a < c; ++a) {
            const long long ij = ecc_pose_scatter::position(u, a, M.data(), n);
            if (ij == ecc_pose_scatter::HOLE) continue;
            ++entries;
            check(ij >= 0 && ij < (long long)n * (n - 1) / 2, "position in range", n, ij);
            check(got.insert(ij).second, "position taken twice", n, ij);
        }
    std::set<long long> want;
    std::vector<char> is_changed((size_t)n, 0);
    for (int v : M) is_changed[v] = 1;
    long long ij = 0;
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j, ++ij)
            if (is_changed[i] || is_changed[j]) want.insert(ij);
    check(got == want, "positions are the pairs of the changed views", n, c);
    check(entries == fb::base_pairs(fb::REFRESH, n, c), "base_pairs of a refresh", n, c);
}

}  // namespace

int main()
{
    for (int n : {4, 5, 8, 12, 16, 40, 127, 128, 400}) check_decide(n);
    check(fb::limit(3) == 0 && fb::limit(16) == 4 && fb::limit(40) == 10 && fb::limit(400) == 32, "limit values");
    check(fb::base_pairs(fb::REFRESH, 16, 1) == 15 && fb::base_pairs(fb::REFRESH, 16, 2) == 29 && fb::base_pairs(fb::REFRESH, 16, 4) == 54 &&
              fb::base_pairs(fb::REFRESH, 40, 8) == 284,
          "base_pairs values");
    for (const auto& M : std::vector<std::vector<int>>{{0}, {11}, {0, 11}, {3, 4, 5}}) check_positions(12, M);
    check_positions(2, {0});
    check_positions(2, {1});
    check_positions(2, {0, 1});
    check_positions(5, {1, 3});
    check_positions(40, {0, 5, 6, 7, 20, 21, 38, 39});
    {
        std::vector<int> M;
        for (int a = 0; a < 32; ++a) M.push_back(3 * a + (a & 1));
        check_positions(127, M);
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("form base ok\n");
    return 0;
}
