// Host-side 256-bit prime-field helpers (4 x u64 limbs, Montgomery R = 2^256).
// Used only off the data path: parameter generation (Grain LFSR, Cauchy MDS), Montgomery constants,
// config validation and canonical<->Montgomery conversion.  The batch data path is HIP-only.
#pragma once
#include <cstdint>
#include <cstring>

namespace pmx {

typedef unsigned __int128 u128;

struct U256 {
    uint64_t l[4];
};

inline bool u256_geq(const U256 &a, const U256 &b) {
    for (int i = 3; i >= 0; --i)
        if (a.l[i] != b.l[i]) return a.l[i] > b.l[i];
    return true;
}

inline bool u256_is_zero(const U256 &a) { return (a.l[0] | a.l[1] | a.l[2] | a.l[3]) == 0; }

// r = a - b, returns borrow
inline uint64_t u256_sub(U256 &r, const U256 &a, const U256 &b) {
    uint64_t borrow = 0;
    for (int i = 0; i < 4; ++i) {
        u128 d = (u128)a.l[i] - b.l[i] - borrow;
        r.l[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
    return borrow;
}

// r = a + b, returns carry
inline uint64_t u256_add(U256 &r, const U256 &a, const U256 &b) {
    uint64_t carry = 0;
    for (int i = 0; i < 4; ++i) {
        u128 s = (u128)a.l[i] + b.l[i] + carry;
        r.l[i] = (uint64_t)s;
        carry = (uint64_t)(s >> 64);
    }
    return carry;
}

struct HostField {
    U256 p;
    uint64_t inv;  // -p^-1 mod 2^64
    U256 r;        // 2^256 mod p  (Montgomery one)
    U256 r2;       // 2^512 mod p

    // p must be odd and > 1.
    bool init(const uint64_t modulus[4]) {
        std::memcpy(p.l, modulus, sizeof p.l);
        if ((p.l[0] & 1) == 0) return false;
        if (p.l[1] == 0 && p.l[2] == 0 && p.l[3] == 0 && p.l[0] < 3) return false;
        // Newton iteration for p^-1 mod 2^64 (doubles the correct bits each step)
        uint64_t x = p.l[0];
        for (int i = 0; i < 6; ++i) x *= 2 - p.l[0] * x;
        inv = (uint64_t)0 - x;
        // r = 2^256 mod p by 256 modular doublings of 1; r2 by 256 more
        U256 v = {{1, 0, 0, 0}};
        if (!u256_geq(p, v)) return false;
        for (int i = 0; i < 256; ++i) v = add(v, v);
        r = v;
        for (int i = 0; i < 256; ++i) v = add(v, v);
        r2 = v;
        return true;
    }

    unsigned bits() const {
        for (int i = 3; i >= 0; --i)
            if (p.l[i]) return 64u * (unsigned)i + (64u - (unsigned)__builtin_clzll(p.l[i]));
        return 0;
    }

    U256 add(const U256 &a, const U256 &b) const {
        U256 s;
        uint64_t c = u256_add(s, a, b);
        if (c || u256_geq(s, p)) u256_sub(s, s, p);
        return s;
    }

    // Montgomery product a*b*2^-256 mod p (word-serial, reduction interleaved)
    U256 mul(const U256 &a, const U256 &b) const {
        uint64_t t[6] = {0, 0, 0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) {
            uint64_t c = 0;
            for (int j = 0; j < 4; ++j) {
                u128 v = (u128)a.l[j] * b.l[i] + t[j] + c;
                t[j] = (uint64_t)v;
                c = (uint64_t)(v >> 64);
            }
            u128 v = (u128)t[4] + c;
            t[4] = (uint64_t)v;
            t[5] = (uint64_t)(v >> 64);
            const uint64_t m = t[0] * inv;
            v = (u128)m * p.l[0] + t[0];
            c = (uint64_t)(v >> 64);
            for (int j = 1; j < 4; ++j) {
                v = (u128)m * p.l[j] + t[j] + c;
                t[j - 1] = (uint64_t)v;
                c = (uint64_t)(v >> 64);
            }
            v = (u128)t[4] + c;
            t[3] = (uint64_t)v;
            t[4] = t[5] + (uint64_t)(v >> 64);
        }
        U256 out = {{t[0], t[1], t[2], t[3]}};
        if (t[4] || u256_geq(out, p)) u256_sub(out, out, p);
        return out;
    }

    U256 neg(const U256 &a) const {
        if (u256_is_zero(a)) return a;
        U256 d;
        u256_sub(d, p, a);
        return d;
    }
    U256 sub(const U256 &a, const U256 &b) const { return add(a, neg(b)); }

    U256 to_mont(const U256 &x) const { return mul(x, r2); }
    U256 from_mont(const U256 &x) const {
        U256 one = {{1, 0, 0, 0}};
        return mul(x, one);
    }

    // x^e in the Montgomery domain, e = the low `bits` bits of the words at `e`
    U256 pow(const U256 &x, const uint64_t *e, int bits) const {
        U256 acc = r;
        for (int bit = bits - 1; bit >= 0; --bit) {
            acc = mul(acc, acc);
            if ((e[bit / 64] >> (bit % 64)) & 1) acc = mul(acc, x);
        }
        return acc;
    }
    U256 pow(const U256 &x, const U256 &e) const { return pow(x, e.l, 256); }
    U256 pow(const U256 &x, uint64_t e) const { return pow(x, &e, 64); }

    // a^(p-2) in the Montgomery domain (Fermat inverse; a != 0)
    U256 inverse(const U256 &a) const {
        U256 e = p, two = {{2, 0, 0, 0}};
        u256_sub(e, e, two);
        return pow(a, e);
    }
};

// ---- number theory over a HostField (values in the Montgomery domain) --------------------------------------------------
inline uint64_t u256_divmod_small(U256 &q, const U256 &a, uint64_t d) {   // q = a / d, returns a % d
    u128 rem = 0;
    for (int i = 3; i >= 0; --i) {
        const u128 cur = (rem << 64) | a.l[i];
        q.l[i] = (uint64_t)(cur / d);
        rem = cur % d;
    }
    return (uint64_t)rem;
}
inline U256 u256_shr(const U256 &a, unsigned k) {   // k < 64
    U256 r;
    for (int i = 0; i < 4; ++i) r.l[i] = k ? ((a.l[i] >> k) | (i + 1 < 4 ? a.l[i + 1] << (64 - k) : 0)) : a.l[i];
    return r;
}
inline bool u256_eq(const U256 &a, const U256 &b) { return a.l[0] == b.l[0] && a.l[1] == b.l[1] && a.l[2] == b.l[2] && a.l[3] == b.l[3]; }
// square root in the Montgomery domain (Tonelli-Shanks); false: a is not a square
inline bool host_sqrt(const HostField &f, const U256 &a, U256 &root) {
    if (u256_is_zero(a)) { root = a; return true; }
    U256 pm1 = f.p;
    pm1.l[0] -= 1;                                   // p odd: no borrow
    unsigned S = 0;
    U256 q = pm1;
    while (!(q.l[0] & 1)) {
        q = u256_shr(q, 1);
        ++S;
    }
    const U256 half = u256_shr(pm1, 1), minus_one = f.neg(f.r);
    if (!u256_eq(f.pow(a, half), f.r)) return false;
    U256 z = f.r;                                    // a non-residue: 2, 3, 4 ... in the Montgomery domain
    for (int tries = 0; tries < 200; ++tries) {
        z = f.add(z, f.r);
        if (u256_eq(f.pow(z, half), minus_one)) break;
        if (tries == 199) return false;
    }
    U256 qp1 = q;                                    // (q + 1) / 2
    qp1.l[0] += 1;                                   // q odd: q + 1 even; no carry unless q = 2^64k - 1 (not for a 225 .. 255-bit p - 1 with S >= 1)
    qp1 = u256_shr(qp1, 1);
    U256 c = f.pow(z, q), r = f.pow(a, qp1), tt = f.pow(a, q);
    unsigned m = S;
    while (!u256_eq(tt, f.r)) {
        unsigned i = 0;
        U256 t2 = tt;
        while (!u256_eq(t2, f.r)) {
            t2 = f.mul(t2, t2);
            if (++i == m) return false;
        }
        U256 b = c;
        for (unsigned k = 0; k + i + 1 < m; ++k) b = f.mul(b, b);
        r = f.mul(r, b);
        c = f.mul(b, b);
        tt = f.mul(tt, c);
        m = i;
    }
    root = r;
    return true;
}
// x^(1/e) for a 64-bit e prime to p - 1 (the map is a bijection): x^d with d = e^-1 mod (p - 1) = (1 + k (p - 1)) / e
inline bool host_root_coprime(const HostField &f, const U256 &x, uint64_t e, U256 &root) {
    if (e == 1) { root = x; return true; }
    U256 pm1 = f.p, Q;
    pm1.l[0] -= 1;
    const uint64_t R = u256_divmod_small(Q, pm1, e);
    // k = -R^-1 mod e (extended Euclid on 64-bit values; no inverse: e shares a factor with p - 1)
    __int128 r0 = (__int128)e, r1 = (__int128)R, t0 = 0, t1 = 1;
    while (r1 != 0) {
        const __int128 q = r0 / r1, r2 = r0 - q * r1, t2 = t0 - q * t1;
        r0 = r1; r1 = r2; t0 = t1; t1 = t2;
    }
    if (r0 != 1) return false;
    __int128 inv = t0 % (__int128)e;
    if (inv < 0) inv += (__int128)e;
    const uint64_t k = (uint64_t)(((__int128)e - inv) % (__int128)e);      // k R = -1 (mod e)
    U256 d = {{0, 0, 0, 0}};                                               // d = k Q + (1 + k R) / e   (k Q < p - 1: no overflow)
    u128 carry = 0;
    for (int i = 0; i < 4; ++i) {
        const u128 v = (u128)Q.l[i] * k + carry;
        d.l[i] = (uint64_t)v;
        carry = v >> 64;
    }
    const u128 rest = ((u128)k * R + 1) / e;
    const U256 add = {{(uint64_t)rest, (uint64_t)(rest >> 64), 0, 0}};
    u256_add(d, d, add);
    root = f.pow(x, d);
    return true;
}
// is x a 2^a-th power?  (the 2-part of p - 1 is 2^S: x^((p - 1) / 2^min(a, S)) = 1)
inline bool host_is_2power_residue(const HostField &f, const U256 &x, unsigned a) {
    if (a == 0 || u256_is_zero(x)) return true;
    U256 e = f.p;
    e.l[0] -= 1;
    for (unsigned i = 0; i < a && !(e.l[0] & 1); ++i) e = u256_shr(e, 1);
    return u256_eq(f.pow(x, e), f.r);
}

}  // namespace pmx
