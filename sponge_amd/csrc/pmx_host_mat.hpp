// Small dense linear algebra over the ABI Montgomery form of a HostField (host only): what the schedule derivations of pmx_derive.hpp
// need - products, the Gauss-Jordan inverse and the rank.
#pragma once
#include <utility>
#include <vector>

#include "pmx_host_field.hpp"

namespace pmx {

typedef std::vector<std::vector<U256>> HostMat;

inline HostMat mat_identity(const HostField &f, size_t n) {
    HostMat m(n, std::vector<U256>(n, U256{{0, 0, 0, 0}}));
    for (size_t i = 0; i < n; ++i) m[i][i] = f.r;
    return m;
}

inline HostMat mat_mul(const HostField &f, const HostMat &a, const HostMat &b) {
    const size_t n = a.size(), k = b.size(), m = b[0].size();
    HostMat r(n, std::vector<U256>(m, U256{{0, 0, 0, 0}}));
    for (size_t i = 0; i < n; ++i)
        for (size_t j = 0; j < m; ++j)
            for (size_t l = 0; l < k; ++l) r[i][j] = f.add(r[i][j], f.mul(a[i][l], b[l][j]));
    return r;
}

inline std::vector<U256> mat_vec(const HostField &f, const HostMat &a, const std::vector<U256> &v) {
    std::vector<U256> r(a.size(), U256{{0, 0, 0, 0}});
    for (size_t i = 0; i < a.size(); ++i)
        for (size_t j = 0; j < v.size(); ++j) r[i] = f.add(r[i], f.mul(a[i][j], v[j]));
    return r;
}

// Gauss-Jordan inverse; false if singular
inline bool mat_inverse(const HostField &f, HostMat a, HostMat &inv) {
    const size_t n = a.size();
    inv = mat_identity(f, n);
    for (size_t col = 0; col < n; ++col) {
        size_t piv = col;
        while (piv < n && u256_is_zero(a[piv][col])) ++piv;
        if (piv == n) return false;
        std::swap(a[piv], a[col]);
        std::swap(inv[piv], inv[col]);
        const U256 d = f.inverse(a[col][col]);
        for (size_t j = 0; j < n; ++j) {
            a[col][j] = f.mul(a[col][j], d);
            inv[col][j] = f.mul(inv[col][j], d);
        }
        for (size_t i = 0; i < n; ++i) {
            if (i == col || u256_is_zero(a[i][col])) continue;
            const U256 k = a[i][col];
            for (size_t j = 0; j < n; ++j) {
                a[i][j] = f.sub(a[i][j], f.mul(k, a[col][j]));
                inv[i][j] = f.sub(inv[i][j], f.mul(k, inv[col][j]));
            }
        }
    }
    return true;
}

inline size_t mat_rank(const HostField &f, HostMat a) {
    size_t rank = 0;
    const size_t n = a.size(), m = n ? a[0].size() : 0;
    for (size_t col = 0; col < m && rank < n; ++col) {
        size_t piv = rank;
        while (piv < n && u256_is_zero(a[piv][col])) ++piv;
        if (piv == n) continue;
        std::swap(a[piv], a[rank]);
        const U256 d = f.inverse(a[rank][col]);
        for (size_t i = rank + 1; i < n; ++i) {
            if (u256_is_zero(a[i][col])) continue;
            const U256 k = f.mul(a[i][col], d);
            for (size_t j = col; j < m; ++j) a[i][j] = f.sub(a[i][j], f.mul(k, a[rank][j]));
        }
        ++rank;
    }
    return rank;
}

}  // namespace pmx
