// depth_dump.cpp — CreateDataSet.output_block_partition_map (CreateDataSet.py:188-264): the partition dump of the patched VTM
// decoder (Save_Depth_fal, Lib/DecoderLib/DecLib.cpp:998-1050) -> the label blocks qt8 / bt16 / dire16 (include/pmp.h).
// Host only: no context, no GPU.  Everything is parsed into temporaries first; the outputs are written only if the whole file is valid.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "pmp_hostonly.h"

namespace {

// One field: a non-negative decimal integer of at most 18 digits (Python's int() accepts more forms; the decoder writes only these).
bool field(const char *&p, const char *end, long long &v)
{
    const char *q = p;
    v = 0;
    while (q < end && *q >= '0' && *q <= '9' && q - p < 18) v = v * 10 + (*q++ - '0');
    if (q == p || (q < end && *q >= '0' && *q <= '9')) return false;
    p = q;
    return true;
}

// "x y h w depth qtDepth btDepth mtDepth s0 .. s7", single spaces, trailing whitespace allowed
bool parse_cu(const char *p, const char *end, long long (&v)[16])
{
    for (int i = 0; i < 16; ++i) {
        if (i > 0) {
            if (p >= end || *p != ' ') return false;
            ++p;
        }
        if (!field(p, end, v[i])) return false;
    }
    for (; p < end; ++p)
        if (*p != ' ' && *p != '\t' && *p != '\r' && *p != '\n') return false;
    return true;
}

}  // namespace

using pmp::set_err_global;

extern "C" int pmp_read_depth_dump(const char *path, int frames, int height, int width, int is_chroma, uint8_t *qt8, uint8_t *bt16,
                                   int8_t *dire16, int64_t *n_unknown)
{
    if (!path || frames < 0 || height < 0 || width < 0)
        return set_err_global(PMP_E_INVALID, "pmp_read_depth_dump: bad arguments");
    const int64_t bh = height / 64, bw = width / 64, nblk = (int64_t)frames * bh * bw;
    if (nblk > 0 && (!qt8 || !bt16 || !dire16)) return set_err_global(PMP_E_INVALID, "pmp_read_depth_dump: null output");
    FILE *f = fopen(path, "rb");
    if (!f) return set_err_global(PMP_E_IO, std::string("pmp_read_depth_dump: cannot open ") + path);
    std::string text;
    {
        char buf[1 << 16];
        size_t got;
        while ((got = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, got);
        const bool bad = ferror(f) != 0;
        fclose(f);
        if (bad) return set_err_global(PMP_E_IO, std::string("pmp_read_depth_dump: read error on ") + path);
    }
    const int64_t R = height / 4, Cc = width / 4, plane = R * Cc;
    std::vector<uint8_t> qm((size_t)(frames * plane)), bm((size_t)(frames * plane));
    std::vector<int8_t> dm((size_t)(frames * 3 * plane));
    const long long factor = is_chroma ? 2 : 1;
    int64_t unknown = 0, frm = -1, lineno = 0;
    size_t pos = 0;
    while (pos < text.size()) {
        size_t eol = text.find('\n', pos);
        const size_t next = eol == std::string::npos ? text.size() : eol + 1;
        if (eol == std::string::npos) eol = text.size();
        const char *b = text.data() + pos, *e = text.data() + eol;
        pos = next;
        ++lineno;
        const std::string where = "pmp_read_depth_dump: line " + std::to_string(lineno);
        if (std::string(b, e).find("frame") != std::string::npos) {        // `if 'frame' in line` (:196)
            if (++frm >= frames) return set_err_global(PMP_E_INVALID, where + ": more frame markers than frames");
            continue;
        }
        if (frm < 0) return set_err_global(PMP_E_INVALID, where + ": CU line before the first frame marker");
        long long v[16];
        if (!parse_cu(b, e, v)) return set_err_global(PMP_E_INVALID, where + ": malformed (16 non-negative integers expected)");
        const long long qd = v[5], bd = v[6];
        if (qd > 5) return set_err_global(PMP_E_INVALID, where + ": qtDepth above 5 (the split code s[qtDepth + 2] does not exist)");
        if (bd > 255) return set_err_global(PMP_E_INVALID, where + ": btDepth outside u8");
        const long long x = v[0] * factor, y = v[1] * factor, h = v[2] * factor, w = v[3] * factor;
        // numpy slices [y//4:(y+h)//4, x//4:(x+w)//4], clipped to the matrix
        auto clip = [](long long a, long long n) { return a < n ? a : n; };
        const int64_t r0 = clip(y / 4, R), r1 = clip((y + h) / 4, R), c0 = clip(x / 4, Cc), c1 = clip((x + w) / 4, Cc);
        int dirs[3], d = 0;
        for (int i = 0; i < 3; ++i) {
            const long long sm = v[8 + qd + i];
            if (sm == 2 || sm == 4) d = 1;
            else if (sm == 3 || sm == 5) d = -1;
            else if (sm == 2000) d = 0;
            else ++unknown;                     // print('Error!!'): the previous layer's direction stays
            dirs[i] = d;
        }
        for (int64_t r = r0; r < r1; ++r)
            for (int64_t c = c0; c < c1; ++c) {
                const size_t o = (size_t)(frm * plane + r * Cc + c);
                qm[o] = (uint8_t)qd;
                bm[o] = (uint8_t)bd;
                for (int i = 0; i < 3; ++i) dm[(size_t)((frm * 3 + i) * plane + r * Cc + c)] = (int8_t)dirs[i];
            }
    }
    // cut (:236-255): qt down-sampled [::2, ::2] to 8x8 per block, bt and dire 16x16
    int64_t blk = 0;
    for (int64_t fr = 0; fr < frames; ++fr)
        for (int64_t i = 0; i < bh; ++i)
            for (int64_t j = 0; j < bw; ++j, ++blk) {
                for (int r = 0; r < 8; ++r)
                    for (int c = 0; c < 8; ++c) qt8[blk * 64 + r * 8 + c] = qm[(size_t)(fr * plane + (2 * (i * 8 + r)) * Cc + 2 * (j * 8 + c))];
                for (int r = 0; r < 16; ++r)
                    for (int c = 0; c < 16; ++c) {
                        const int64_t rr = i * 16 + r, cc = j * 16 + c;
                        bt16[blk * 256 + r * 16 + c] = bm[(size_t)(fr * plane + rr * Cc + cc)];
                        for (int k = 0; k < 3; ++k) dire16[(blk * 3 + k) * 256 + r * 16 + c] = dm[(size_t)((fr * 3 + k) * plane + rr * Cc + cc)];
                    }
            }
    if (n_unknown) *n_unknown = unknown;
    return PMP_OK;
}
