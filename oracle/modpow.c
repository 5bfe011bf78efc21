/* x^e mod p for many x of up to 256 bits  --  TEST INFRASTRUCTURE ONLY (oracle/inverse.py).
 *
 * The inverse S-box of a planted state is x^(alpha^-1 mod p-1): an exponent as long as the modulus, about 120 us a root with Python
 * integers and some hundred thousand roots for the plants of one t = 9 config.  This file is that one loop in C (Montgomery form, four
 * 64-bit limbs, binary exponentiation); oracle/inverse.py compiles it on demand and falls back to pow() where no compiler is found.
 * Nothing here decides an expected value: tests/plants.py checks every plant with the Python oracle's forward walk, so a wrong root
 * could only make a plant miss.
 */
#include <stddef.h>
#include <stdint.h>

typedef unsigned __int128 u128;

/* r = a * b * 2^-256 mod p, r < p for a, b < p; inv = -p^-1 mod 2^64; p odd and below 2^255 */
static void mont_mul(uint64_t r[4], const uint64_t a[4], const uint64_t b[4], const uint64_t p[4], uint64_t inv) {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int j = 0; j < 4; j++) {
            c += (u128)a[j] * b[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        uint64_t m = t[0] * inv;
        c = ((u128)m * p[0] + t[0]) >> 64;
        for (int j = 1; j < 4; j++) {
            c += (u128)m * p[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    uint64_t d[4], borrow = 0;
    for (int j = 0; j < 4; j++) {
        u128 s = (u128)t[j] - p[j] - borrow;
        d[j] = (uint64_t)s;
        borrow = (uint64_t)(s >> 64) & 1;
    }
    int keep = t[4] == 0 && borrow;         /* t < p: the difference went below zero */
    for (int j = 0; j < 4; j++) r[j] = keep ? t[j] : d[j];
}

/* x [n][4] little-endian limbs, each below p, replaced by x^e mod p; r2 = 2^512 mod p */
int modpow_batch(uint64_t *x, size_t n, const uint64_t e[4], const uint64_t p[4], const uint64_t r2[4], uint64_t inv) {
    const uint64_t one[4] = {1, 0, 0, 0};
    uint64_t mont_one[4];
    int top = -1;
    for (int k = 255; k >= 0; k--)
        if ((e[k / 64] >> (k % 64)) & 1) { top = k; break; }
    mont_mul(mont_one, one, r2, p, inv);
    for (size_t i = 0; i < n; i++) {
        uint64_t base[4], acc[4];
        mont_mul(base, x + 4 * i, r2, p, inv);
        for (int j = 0; j < 4; j++) acc[j] = mont_one[j];
        for (int k = top; k >= 0; k--) {
            mont_mul(acc, acc, acc, p, inv);
            if ((e[k / 64] >> (k % 64)) & 1) mont_mul(acc, acc, base, p, inv);
        }
        mont_mul(x + 4 * i, acc, one, p, inv);
    }
    return 0;
}
