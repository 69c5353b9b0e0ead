// Small host-side helpers shared by bdg_chunks.cpp, stage1.cpp and tsv_io.cpp: the clock, text output of numbers and barcodes,
// write(2) to the end.
#pragma once

#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <cstddef>
#include <cstdint>

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline char* put_uint(char* o, uint32_t u)
{
    char t[12]; int k = 0;
    do { t[k++] = (char)('0' + u % 10); u /= 10; } while (u);
    while (k) *o++ = t[--k];
    return o;
}

inline char* put_int(char* o, int v)
{
    if (v < 0) *o++ = '-';
    return put_uint(o, v < 0 ? 0u - (unsigned)v : (unsigned)v);
}

// the 16 letters of a barcode's rank (unrank, common.py:27-38: the first letter in the lowest two bits)
inline char* put_barcode16(char* o, uint32_t rank)
{
    for (int b = 0; b < 16; ++b) *o++ = "ACGT"[(rank >> (2 * b)) & 3u];
    return o;
}

// the letters of a packed UMI code (len << 28 | 2-bit letters, first letter most significant; bdg_extract_keep_umis)
inline char* put_umi_code(char* o, uint32_t c)
{
    const uint32_t L = c >> 28;
    for (uint32_t j = 0; j < L; ++j) *o++ = "ACGT"[(c >> (2 * (L - 1 - j))) & 3u];
    return o;
}

// 0 .. 3 for A, C, G, T; 4 for every other letter
inline uint32_t acgt_code(char c)
{
    switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return 4; }
}

inline bool write_all(int fd, const char* p, size_t n)
{
    while (n) {
        const ssize_t w = ::write(fd, p, n);
        if (w < 0) { if (errno == EINTR) continue; return false; }
        p += w; n -= (size_t)w;
    }
    return true;
}
