// The live overlay of one frame as primitive lists (overlay.py::LiveVisualizer), written once for the build kernel
// (live_overlay.hip), for the host entry vc_overlay_build_host and for the host build the CPU tests compile
// (tests/native/overlay_build_host.cpp).  No HIP, no allocation, no library call but rint.
//
// It restates overlay.py::PrimList call by call -- draw_anno, draw_arrow + draw_one_box per row, draw_text, draw_frame_count -- on
// the 12-int32 primitives overlay_kernel paints (overlay.hip): [type, x0, y0, x1, y1, t, colour, glyph bits lo, glyph bits hi, 0, 0, 0].
// A frame is a sequence of PARTS, each a function of the batch's inputs alone:
//   anno | one part per in-zone row | count text: per direction line {outline pass, fill pass} x {head, one segment per label} | frame number
// Every part has ONE body, emit_*(Out&, ...): with Out::p null it only counts (count_* below), so a count cannot disagree with what
// is written.
//
// Python arithmetic that is restated here: int(x) truncates towards zero; round(x) rounds half to even (rint in the default rounding
// mode); a primitive field is the value modulo 2^32 (PrimList._add -> uint32 -> int32).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VC_OB_HD __host__ __device__ inline
#else
#define VC_OB_HD inline
#endif

namespace vc {
namespace ob {

enum { LINE = 0, DISC = 1, RECT = 2, FILL = 3, GLYPH = 4 };
enum { GLYPH_W = 5, GLYPH_H = 7, GLYPH_ADV = 6 };
enum { WHITE = 0xFFFFFF, BLACK = 0, RED = 0xFF0000, GREEN = 0x00FF00 };     // B | G << 8 | R << 16
enum { OB_MAX_DIRS = 16 };                                                   // = cc::CC_MAX_DIRS: the stride of dir_lines / dir_keys per camera

// overlay.py::_F: 35-bit bitmap, bit 5 * row + column, rows top to bottom; lower case draws as capitals, an unknown character as '?'
VC_OB_HD uint64_t glyph_bits(int ch) {
    if (ch >= 'a' && ch <= 'z') ch -= 32;
    switch (ch) {
    case ' ': return 0x0ull; case '0': return 0x3A33AE62Eull; case '1': return 0x3884210C4ull; case '2': return 0x7C444422Eull;
    case '3': return 0x3A304111Full; case '4': return 0x211F4A988ull; case '5': return 0x3A3083C3Full;
    case '6': return 0x3A317844Cull; case '7': return 0x8422221Full; case '8': return 0x3A317462Eull;
    case '9': return 0x1910F462Eull; case 'A': return 0x4631FC62Eull; case 'B': return 0x3E317C62Full;
    case 'C': return 0x3A210862Eull; case 'D': return 0x1D318C527ull; case 'E': return 0x7C217843Full;
    case 'F': return 0x4217843Full; case 'G': return 0x7A31E862Eull; case 'H': return 0x4631FC631ull;
    case 'I': return 0x38842108Eull; case 'J': return 0x19284211Cull; case 'K': return 0x452519531ull;
    case 'L': return 0x7C2108421ull; case 'M': return 0x4631AD771ull; case 'N': return 0x4639ACE31ull;
    case 'O': return 0x3A318C62Eull; case 'P': return 0x4217C62Full; case 'Q': return 0x59358C62Eull;
    case 'R': return 0x45257C62Full; case 'S': return 0x3E107043Eull; case 'T': return 0x10842109Full;
    case 'U': return 0x3A318C631ull; case 'V': return 0x11518C631ull; case 'W': return 0x2AB5AC631ull;
    case 'X': return 0x462A22A31ull; case 'Y': return 0x108454631ull; case 'Z': return 0x7C222221Full; case ':': return 0x8401080ull;
    case '|': return 0x108421084ull; case '.': return 0x18C000000ull; case '-': return 0xF8000ull; case '_': return 0x7C0000000ull;
    case ',': return 0x88600000ull; case '/': return 0x42222210ull;
    default: return 0x10044422Eull;                                          // '?'
    }
}

// overlay.py::text_scale: max(1, int(round(2 * font_scale)))
VC_OB_HD int text_scale(double font_scale) {
    const int s = (int)rint(2.0 * font_scale);
    return s > 1 ? s : 1;
}
// overlay.py::text_size of a line of `len` characters: (width, height)
VC_OB_HD int text_width(int len, int scale) { return (len * GLYPH_ADV - 1 > 0 ? len * GLYPH_ADV - 1 : 0) * scale; }
VC_OB_HD int text_height(int scale) { return GLYPH_H * scale; }

// str(v) into buf (room for 20 characters), returns its length
VC_OB_HD int fmt_i64(int64_t v, char* buf) {
    uint64_t u = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    char tmp[20];
    int n = 0;
    do { tmp[n++] = (char)('0' + (int)(u % 10)); u /= 10; } while (u);
    int k = 0;
    if (v < 0) buf[k++] = '-';
    while (n) buf[k++] = tmp[--n];
    return k;
}
VC_OB_HD int digits_i64(int64_t v) { char b[20]; return fmt_i64(v, b); }

// overlay.py::track_color, packed as PrimList._add packs it
VC_OB_HD int track_color(int64_t label, int64_t track_id) {
    uint32_t x = (uint32_t)(uint64_t)label * 0x9E3779B1u + (uint32_t)(uint64_t)track_id * 0x85EBCA6Bu + 0x27D4EB2Fu;
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    return (int)((64 + (x & 127)) | ((64 + ((x >> 8) & 127)) << 8) | ((64 + ((x >> 16) & 127)) << 16));
}

// draw_one_box's line thickness: int(round(0.001 * max(h, w))) or 1
VC_OB_HD int box_tl(int h, int w) {
    const int tl = (int)rint(0.001 * (double)(h > w ? h : w));
    return tl ? tl : 1;
}
// int((a + b) / 2) on Python's true division
VC_OB_HD int64_t mid(int64_t a, int64_t b) { return (int64_t)((double)(a + b) / 2); }

// Where primitives go.  p null: count only; else 16-byte aligned (a primitive is 48 bytes: three 16-byte stores each).
struct Out {
    int32_t* p;
    int n;
};
struct alignas(16) Prim12 { int32_t v[12]; };
VC_OB_HD void put(Out& o, int type, int64_t x0, int64_t y0, int64_t x1, int64_t y1, int t, int color, uint64_t bits) {
    if (o.p) {
        Prim12 q;
        q.v[0] = type; q.v[1] = (int32_t)(uint32_t)(uint64_t)x0; q.v[2] = (int32_t)(uint32_t)(uint64_t)y0; q.v[3] = (int32_t)(uint32_t)(uint64_t)x1;
        q.v[4] = (int32_t)(uint32_t)(uint64_t)y1; q.v[5] = t; q.v[6] = color; q.v[7] = (int32_t)(uint32_t)(bits & 0xFFFFFFFFull);
        q.v[8] = (int32_t)(uint32_t)(bits >> 32); q.v[9] = 0; q.v[10] = 0; q.v[11] = 0;
        *(Prim12*)(o.p + (size_t)o.n * 12) = q;
    }
    ++o.n;
}

// PrimList.text for the characters s[0, len) that stand at positions pos0 .. of a line whose bottom-left corner is (x, y_bottom)
VC_OB_HD void emit_text(Out& o, const char* s, int len, int pos0, int64_t x, int64_t y_bottom, int scale, int color, int bold) {
    const int64_t y = y_bottom - GLYPH_H * scale;
    for (int i = 0; i < len; ++i) {
        const uint64_t bits = glyph_bits((unsigned char)s[i]);
        if (bits == 0) continue;
        const int64_t gx = x + (int64_t)(pos0 + i) * GLYPH_ADV * scale;
        for (int oy = -bold; oy <= bold; ++oy)
            for (int ox = -bold; ox <= bold; ++ox) put(o, GLYPH, gx + ox, y + oy, 0, 0, scale, color, bits);
    }
}

VC_OB_HD void emit_arrow(Out& o, int64_t x0, int64_t y0, int64_t x1, int64_t y1, int color) {
    put(o, LINE, x0, y0, x1, y1, 3, color, 0);
    put(o, DISC, x1, y1, 0, 0, 8, color, 0);
}

// ---- part: anno (PrimList.draw_anno) -----------------------------------------------------------------------------------------------
// polygon_xy: pn points; dir_lines: n_dir x (x0, y0, x1, y1); dir_keys: the directions' names as numbers, drawn with two digits as
// the zone file spells them ("direction01" -> "01")
VC_OB_HD void emit_anno(Out& o, const double* polygon_xy, int pn, const double* dir_lines, int n_dir, const int* dir_keys) {
    for (int i = 0; i < pn; ++i) {
        const int j = i + 1 == pn ? 0 : i + 1;
        put(o, LINE, (int64_t)polygon_xy[i * 2], (int64_t)polygon_xy[i * 2 + 1], (int64_t)polygon_xy[j * 2], (int64_t)polygon_xy[j * 2 + 1], 5, RED, 0);
    }
    for (int d = 0; d < n_dir; ++d) {
        const double* l = dir_lines + (size_t)d * 4;
        const int64_t x1 = (int64_t)l[2], y1 = (int64_t)l[3];
        emit_arrow(o, (int64_t)l[0], (int64_t)l[1], x1, y1, BLACK);
        char s[21];
        int n = 0;
        if (dir_keys[d] >= 0 && dir_keys[d] < 10) s[n++] = '0';
        n += fmt_i64(dir_keys[d], s + n);
        emit_text(o, s, n, 0, x1, y1, text_scale(1.5), BLACK, 1);
    }
}

// ---- part: one in-zone row (PrimList.visualize_one_frame's body) --------------------------------------------------------------------
// box: the row's own; first: the first in-zone box of its track
VC_OB_HD void emit_row(Out& o, int h, int w, const int64_t* box, const int64_t* first, int64_t track_id, int64_t label) {
    const int color = track_color(label, track_id);
    emit_arrow(o, mid(first[0], first[2]), mid(first[1], first[3]), mid(box[0], box[2]), mid(box[1], box[3]), color);
    const int tl = box_tl(h, w);
    put(o, RECT, box[0], box[1], box[2], box[3], tl * 2, color, 0);
    char s[64];                                                        // "id: <id> || cls: <label>"
    int n = 0;
    s[n++] = 'i'; s[n++] = 'd'; s[n++] = ':'; s[n++] = ' ';
    const int dt = fmt_i64(track_id, s + n); n += dt;
    s[n++] = ' '; s[n++] = '|'; s[n++] = '|'; s[n++] = ' '; s[n++] = 'c'; s[n++] = 'l'; s[n++] = 's'; s[n++] = ':'; s[n++] = ' ';
    const int dl = fmt_i64(label, s + n); n += dl;
    const int scale = text_scale((double)tl / 3);
    const int t_w = text_width(4 + dt + 2, scale), s_w = text_width(7 + dl, scale);        // "id: <id> |" and "| cls: <label>"
    put(o, FILL, box[0], box[1], box[0] + t_w + s_w + 15, box[1] - text_height(scale) - 3, 0, color, 0);
    emit_text(o, s, n, 0, box[0], box[1] - 2, scale, BLACK, 0);
}

// ---- part: count text (PrimList.draw_text on count_frame_directions' text, default position) ----------------------------------------
// Line d of n_dir is "direction:<key> || " (segment 0) followed by "<label>:<count> | " for every label (segment 1 + label); it is
// painted as an outline pass (black, 9 offsets) and then a fill pass (white).  counts_d: the n_labels counts of this direction.
enum { TEXT_PASSES = 2 };
VC_OB_HD int text_parts(int n_dir, int n_labels) { return n_dir * TEXT_PASSES * (1 + n_labels); }
VC_OB_HD int seg_chars(int seg, int key, const int32_t* counts_d, char* s) {
    int n = 0;
    if (seg == 0) {
        const char head[] = "direction:";
        for (int i = 0; i < 10; ++i) s[n++] = head[i];
        n += fmt_i64(key, s + n);
        s[n++] = ' '; s[n++] = '|'; s[n++] = '|'; s[n++] = ' ';
    } else {
        n += fmt_i64(seg - 1, s + n);
        s[n++] = ':';
        n += fmt_i64(counts_d[seg - 1], s + n);
        s[n++] = ' '; s[n++] = '|'; s[n++] = ' ';
    }
    return n;
}
VC_OB_HD void emit_count_seg(Out& o, int h, int n_dir, int d, int key, const int32_t* counts_d, int pass, int seg) {
    const int scale = text_scale(0.75), hl = text_height(scale);
    int pos = 0;
    if (seg > 0) {
        pos = 10 + digits_i64(key) + 4;
        for (int l = 0; l + 1 < seg; ++l) pos += digits_i64(l) + 1 + digits_i64(counts_d[l]) + 3;
    }
    char s[40];
    const int n = seg_chars(seg, key, counts_d, s);
    // v starts at h - hl * (lines + 3) and advances by hl * 1.5 per line; hl is even at every scale text_scale(0.75) gives (2)
    const int64_t v = (int64_t)h - (int64_t)hl * (n_dir + 3) + (int64_t)(hl * 3 / 2) * d;
    emit_text(o, s, n, pos, 10, v + hl, scale, pass == 0 ? BLACK : WHITE, pass == 0 ? 1 : 0);
}
// part index within the text -> (direction line, pass, segment), in painting order
VC_OB_HD void text_part(int part, int n_labels, int* d, int* pass, int* seg) {
    const int per_pass = 1 + n_labels;
    *d = part / (TEXT_PASSES * per_pass);
    *pass = part / per_pass % TEXT_PASSES;
    *seg = part % per_pass;
}

// ---- part: frame number (PrimList.draw_frame_count) ----------------------------------------------------------------------------------
VC_OB_HD void emit_frame_no(Out& o, int64_t frame_no) {
    char s[32];
    const char head[] = "Frame:";
    int n = 0;
    for (int i = 0; i < 6; ++i) s[n++] = head[i];
    n += fmt_i64(frame_no, s + n);
    const int scale = text_scale(0.75);
    emit_text(o, s, n, 0, 10, 25 + text_height(scale), scale, BLACK, 1);
    emit_text(o, s, n, 0, 10, 25 + text_height(scale), scale, GREEN, 0);
}

// ---- counts: the same bodies without a destination ---------------------------------------------------------------------------------
VC_OB_HD int count_anno(const double* polygon_xy, int pn, const double* dir_lines, int n_dir, const int* dir_keys) {
    Out o{nullptr, 0};
    emit_anno(o, polygon_xy, pn, dir_lines, n_dir, dir_keys);
    return o.n;
}
VC_OB_HD int count_row(int64_t track_id, int64_t label) {              // a row's count depends on the digits of its id and label alone
    const int64_t zero[4] = {0, 0, 0, 0};
    Out o{nullptr, 0};
    emit_row(o, 1, 1, zero, zero, track_id, label);
    return o.n;
}
VC_OB_HD int count_count_seg(int key, const int32_t* counts_d, int pass, int seg) {
    Out o{nullptr, 0};
    emit_count_seg(o, 0, 1, 0, key, counts_d, pass, seg);
    return o.n;
}
VC_OB_HD int count_frame_no(int64_t frame_no) {
    Out o{nullptr, 0};
    emit_frame_no(o, frame_no);
    return o.n;
}

// ---- one whole frame, part after part (the host form; the kernel spreads the same parts over its lanes) ------------------------------
// rows6 / first4: the frame's n_rows rows in emit order with the first in-zone box of each row's track; keep[i] != 0: the row has a
// corner in the zone.  counts_cam: [max_dir][n_labels] of this camera before the batch, null = no text.
VC_OB_HD void emit_frame(Out& o, int h, int w, const double* polygon_xy, int pn, const double* dir_lines, int n_dir, const int* dir_keys, int n_labels,
                         const int32_t* counts_cam, const int64_t* rows6, const int64_t* first4, const unsigned char* keep, int n_rows, int64_t frame_no) {
    emit_anno(o, polygon_xy, pn, dir_lines, n_dir, dir_keys);
    for (int i = 0; i < n_rows; ++i)
        if (keep[i]) emit_row(o, h, w, rows6 + (size_t)i * 6, first4 + (size_t)i * 4, rows6[(size_t)i * 6 + 4], rows6[(size_t)i * 6 + 5]);
    if (counts_cam)
        for (int part = 0; part < text_parts(n_dir, n_labels); ++part) {
            int d, pass, seg;
            text_part(part, n_labels, &d, &pass, &seg);
            emit_count_seg(o, h, n_dir, d, dir_keys[d], counts_cam + (size_t)d * n_labels, pass, seg);
        }
    emit_frame_no(o, frame_no);
}

}  // namespace ob
}  // namespace vc
