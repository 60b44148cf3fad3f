// The two networks as data: the detector (YOLOv5 v6.0 graph) and the ReID net, their parameters, activation buffers and op plans.
// engine_run.hip executes the plans, engine.hip owns the engine and the C ABI.
//
// Graph sources restated here (independently of oracle/yolov5.py, they only meet at the parameter names):
//   ultralytics/yolov5 v6.0 models/yolov5{s,m,l,x}.yaml + models/common.py (Conv, Bottleneck, C3, SPPF, Concat) +
//   models/yolo.py (Detect), loaded by /root/reference/networks/yolo.py:58;
//   /root/reference/networks/deepsort/deep/model.py:5-98 (BasicBlock, make_layers, Net(reid=True)).
// Concat never copies: producers write straight into channel slices of the consumer's buffer.
#include <algorithm>
#include <cmath>

#include "engine.h"

namespace vc {

// ------------------------------------------------------------------------------------------------ plan helpers
View mkview(const View& buf, int B, int H, int W, int C, int co) {
    View v = buf;
    v.B = B; v.H = H; v.W = W; v.C = C; v.co = buf.co + co;
    return v;
}

static int alloc_buf(vc_engine* e, std::map<std::string, View>& m, const std::string& name, size_t pixels, int C, int es) {
    View v{};
    v.cs = C; v.co = 0; v.C = C; v.es = es;
    VC_TRY(dev_alloc(e, &v.ptr, pixels * C * es));
    m[name] = v;
    return VC_OK;
}

ConvP conv_params(const ConvParam& p, ConvSlice in, ConvSlice out, int B, int H, int W, int kh, int kw, int stride, int pad, int act,
                  float act_scale, float inv_act_scale) {
    ConvP c{};
    c.in = in.ptr; c.w = p.d_w; c.bias = p.d_b; c.out = out.ptr;
    c.B = B; c.H = H;
    if (p.pair_stem) {
        c.W = W / 2; c.Cin = 8; c.in_cs = 8; c.in_co = 0;
        c.kh = p.kh; c.kw = p.kw / 2; c.sh = stride; c.sw = 1; c.ph = pad; c.pw = 1;
    } else {
        c.W = W; c.Cin = p.cin_eff; c.in_cs = in.cs; c.in_co = in.co;
        c.kh = kh; c.kw = kw; c.sh = c.sw = stride; c.ph = c.pw = pad;
    }
    c.Ho = (H + 2 * pad - kh) / stride + 1; c.Wo = (W + 2 * pad - kw) / stride + 1;
    c.Cout = p.O; c.out_cs = out.cs; c.out_co = out.co;
    c.K = p.K; c.Kp = p.Kp;
    c.act = act; c.res_mode = RES_NONE; c.prec = p.prec;
    c.scale = p.d_scale; c.act_scale = act_scale; c.inv_act_scale = inv_act_scale;
    c.M = B * c.Ho * c.Wo;
    c.cfg = -1;
    return c;
}

struct PlanBuilder {
    vc_engine* e;
    Net* net;
    std::vector<Op>* ops;
    int prec;
    int status = VC_OK;

    // out.H/W are filled from the conv arithmetic; returns the output view with its dims set
    View conv(const std::string& pname, View in, View out, int k, int s, int p, int act, const View* res = nullptr,
              int res_mode = RES_NONE, bool out_f32 = false) {
        auto it = net->index.find(pname);
        if (it == net->index.end()) { set_error("plan: unknown parameter %s", pname.c_str()); status = VC_ERR_NOTFOUND; return out; }
        const ConvParam& cp = net->params[it->second];
        Op op{};
        op.kind = Op::CONV;
        op.param = it->second;
        ConvP& c = op.conv;
        c = conv_params(cp, {in.ptr, in.cs, in.co}, {out.ptr, out.cs, out.co}, in.B, in.H, in.W, k, k, s, p, act, e->act_scale, 1.0f / e->act_scale);
        c.res_mode = res_mode; c.out_f32 = out_f32 ? 1 : 0;
        if (res) { c.res = res->ptr; c.res_cs = res->cs; c.res_co = res->co; }
        op.C = cp.I * cp.kh * cp.kw;          // logical K for algorithmic FLOPs
        ops->push_back(op);
        out.B = in.B; out.H = c.Ho; out.W = c.Wo; out.C = cp.O;
        return out;
    }
};

// ------------------------------------------------------------------------------------------------ YOLOv5 v6.0
static const double kYoloMult[4][2] = {{0.33, 0.50}, {0.67, 0.75}, {1.0, 1.0}, {1.33, 1.25}};   // depth, width (s, m, l, x)
const float kAnchors[3][6] = {{10, 13, 16, 30, 33, 23}, {30, 61, 62, 45, 59, 119}, {116, 90, 156, 198, 373, 326}};

static void yolo_c3_params(Net& n, int idx, int cin, int cout, int reps) {
    const std::string p = "model." + std::to_string(idx);
    const int h = cout / 2;
    const int a = n.add(p + ".cv1.conv", h, cin, 1, 1);
    const int b = n.add(p + ".cv2.conv", h, cin, 1, 1);
    n.add(p + ".cv3.conv", cout, 2 * h, 1, 1);
    const int f = n.add(p + ".cv12", 2 * h, cin, 1, 1);        // cv1 and cv2 read the same input: one launch, two destinations
    n.params[f].fuse_a = a; n.params[f].fuse_b = b; n.params[f].hidden = true;
    for (int j = 0; j < reps; ++j) {
        n.add(p + ".m." + std::to_string(j) + ".cv1.conv", h, h, 1, 1);
        n.add(p + ".m." + std::to_string(j) + ".cv2.conv", h, h, 3, 3);
    }
}

void yolo_define(vc_engine* e) {
    const double gd = kYoloMult[e->cfg.yolo_variant][0], gw = kYoloMult[e->cfg.yolo_variant][1];
    const int base[5] = {64, 128, 256, 512, 1024};
    for (int i = 0; i < 5; ++i) e->ch[i] = (int)std::ceil(base[i] * gw / 8.0) * 8;
    const int r[4] = {3, 6, 9, 3};
    for (int i = 0; i < 4; ++i) e->rep[i] = std::max((int)std::nearbyint(r[i] * gd), 1);
    Net& n = e->yolo;
    const int* c = e->ch;
    n.add("model.0.conv", c[0], 3, 6, 6);
    n.params.back().pair_stem = (e->aux_prec == PREC_BF16);       // the stem stays bf16 in the fp8 mode
    n.add("model.1.conv", c[1], c[0], 3, 3); yolo_c3_params(n, 2, c[1], c[1], e->rep[0]);
    n.add("model.3.conv", c[2], c[1], 3, 3); yolo_c3_params(n, 4, c[2], c[2], e->rep[1]);
    n.add("model.5.conv", c[3], c[2], 3, 3); yolo_c3_params(n, 6, c[3], c[3], e->rep[2]);
    n.add("model.7.conv", c[4], c[3], 3, 3); yolo_c3_params(n, 8, c[4], c[4], e->rep[3]);
    n.add("model.9.cv1.conv", c[4] / 2, c[4], 1, 1);
    n.add("model.9.cv2.conv", c[4], c[4] * 2, 1, 1);
    n.add("model.10.conv", c[3], c[4], 1, 1); yolo_c3_params(n, 13, 2 * c[3], c[3], e->rep[0]);
    n.add("model.14.conv", c[2], c[3], 1, 1); yolo_c3_params(n, 17, 2 * c[2], c[2], e->rep[0]);
    n.add("model.18.conv", c[2], c[2], 3, 3); yolo_c3_params(n, 20, 2 * c[2], c[3], e->rep[0]);
    n.add("model.21.conv", c[3], c[3], 3, 3); yolo_c3_params(n, 23, 2 * c[3], c[4], e->rep[0]);
    const int no = 3 * (e->cfg.num_classes + 5);
    for (int i = 0; i < 3; ++i) {
        const int h = n.add("model.24.m." + std::to_string(i), no, c[2 + i], 1, 1);
        const int o = n.add("model.24.m." + std::to_string(i) + ".obj", 8, c[2 + i], 1, 1);      // sparse head: the three objectness rows, padded to 8
        n.params[o].obj_of = h; n.params[o].hidden = true;
    }
}

int yolo_alloc(vc_engine* e) {
    const int es = elem_size(e->prec), aes = elem_size(e->aux_prec);
    const int S = round_up(e->cfg.img_size, 32);
    const size_t B = e->cfg.max_batch;
    auto px = [&](int stride) { return B * (size_t)(S / stride) * (S / stride); };
    const int* c = e->ch;
    auto& m = e->ybuf;
    auto c3 = [&](int idx, int stride, int cout) -> int {
        const std::string p = "c3_" + std::to_string(idx);
        const int h = cout / 2;
        VC_TRY(alloc_buf(e, m, p + ".a", px(stride), h, es));
        VC_TRY(alloc_buf(e, m, p + ".b", px(stride), h, es));
        VC_TRY(alloc_buf(e, m, p + ".t", px(stride), h, es));
        VC_TRY(alloc_buf(e, m, p + ".cat", px(stride), 2 * h, es));
        return VC_OK;
    };
    VC_TRY(alloc_buf(e, m, "in", px(1), 4, aes));
    VC_TRY(alloc_buf(e, m, "l0", px(2), c[0], aes));
    if (e->prec == PREC_FP8) VC_TRY(alloc_buf(e, m, "l0q", px(2), c[0], es));       // the bf16 stem output converted to fp8
    VC_TRY(alloc_buf(e, m, "l1", px(4), c[1], es)); VC_TRY(c3(2, 4, c[1])); VC_TRY(alloc_buf(e, m, "l2", px(4), c[1], es));
    VC_TRY(alloc_buf(e, m, "l3", px(8), c[2], es)); VC_TRY(c3(4, 8, c[2])); VC_TRY(alloc_buf(e, m, "cat16", px(8), 2 * c[2], es));
    VC_TRY(alloc_buf(e, m, "l5", px(16), c[3], es)); VC_TRY(c3(6, 16, c[3])); VC_TRY(alloc_buf(e, m, "cat12", px(16), 2 * c[3], es));
    VC_TRY(alloc_buf(e, m, "l7", px(32), c[4], es)); VC_TRY(c3(8, 32, c[4])); VC_TRY(alloc_buf(e, m, "l8", px(32), c[4], es));
    VC_TRY(alloc_buf(e, m, "sppcat", px(32), 2 * c[4], es));
    VC_TRY(alloc_buf(e, m, "l9", px(32), c[4], es));
    VC_TRY(alloc_buf(e, m, "cat22", px(32), 2 * c[3], es));
    VC_TRY(c3(13, 16, c[3])); VC_TRY(alloc_buf(e, m, "l13", px(16), c[3], es));
    VC_TRY(alloc_buf(e, m, "cat19", px(16), 2 * c[2], es));
    VC_TRY(c3(17, 8, c[2])); VC_TRY(alloc_buf(e, m, "l17", px(8), c[2], es));
    VC_TRY(c3(20, 16, c[3])); VC_TRY(alloc_buf(e, m, "l20", px(16), c[3], es));
    VC_TRY(c3(23, 32, c[4])); VC_TRY(alloc_buf(e, m, "l23", px(32), c[4], es));
    const int no = 3 * (e->cfg.num_classes + 5);
    const int lcs = round_up(no, 8);
    const int strides[3] = {8, 16, 32};
    for (int i = 0; i < 3; ++i) VC_TRY(dev_alloc(e, (void**)&e->d_logits[i], px(strides[i]) * lcs * sizeof(float)));
    if (e->prec == PREC_BF16) {
        // sparse head: per level an 8-channel objectness plane and room for EVERY pixel of the batch in the gathered list (a
        // pooled B x max_candidates capacity could overflow on one busy frame where the dense head, which only counts anchors with
        // obj x cls > conf against max_candidates per frame, succeeds; 0.6 GB at B = 128 / 640 x 640 of 288 GB buys "cannot overflow")
        for (int i = 0; i < 3; ++i) {
            const size_t ppf = (size_t)(S / strides[i]) * (S / strides[i]);
            e->hc_cap[i] = (int)(B * ppf);
            VC_TRY(dev_alloc(e, &e->d_obj[i], px(strides[i]) * 8 * 2));
            VC_TRY(dev_alloc(e, (void**)&e->d_hc_list[i], (size_t)e->hc_cap[i] * sizeof(int)));
            VC_TRY(dev_alloc(e, &e->d_hc_x[i], (size_t)e->hc_cap[i] * c[2 + i] * 2));
            VC_TRY(dev_alloc(e, &e->d_hc_logits[i], (size_t)e->hc_cap[i] * lcs * 2));
        }
        e->want_hc_count = true;                            // carved out of the zero block below (one memset per pass clears all three)
        VC_TRY(host_alloc(e, (void**)&e->h_hc_ring, (size_t)vc_engine::HC_RING * 4 * sizeof(int)));
        memset(e->h_hc_ring, 0, (size_t)vc_engine::HC_RING * 4 * sizeof(int));
    }
    // post-processing
    const size_t mc = e->cfg.max_candidates, md = e->cfg.max_det;
    auto& pb = e->post;
    VC_TRY(dev_alloc(e, (void**)&pb.cand_box, B * mc * 4 * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&pb.cand_conf, B * mc * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&pb.cand_cls, B * mc * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&pb.cand_idx, B * mc * sizeof(int)));
    // per-pass counters in ONE block: [sparse-head row counts, 64 B][cand_count][overflow] -- a single memset at the head of the detector's
    // chain of dependent launches instead of three
    e->zero_bytes = 64 + 2 * B * sizeof(int);
    VC_TRY(dev_alloc(e, (void**)&e->d_zero, e->zero_bytes));
    if (e->want_hc_count) e->d_hc_count = (int*)e->d_zero;
    pb.cand_count = (int*)((char*)e->d_zero + 64);
    VC_TRY(dev_alloc(e, (void**)&pb.sort_box, B * mc * 4 * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&pb.sort_conf, B * mc * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&pb.sort_cls, B * mc * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&pb.mask, B * mc * (mc / 64) * sizeof(unsigned long long)));
    VC_TRY(dev_alloc(e, (void**)&pb.det, B * md * 6 * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&pb.det_count, B * sizeof(int)));
    pb.overflow = pb.cand_count + B;
    VC_TRY(dev_alloc(e, (void**)&e->d_geom, B * 5 * sizeof(float)));
    VC_TRY(host_alloc(e, (void**)&e->h_geom, 2 * B * 5 * sizeof(float)));
    for (int k = 0; k < 2; ++k) {
        VC_TRY(host_alloc(e, (void**)&e->h_det2[k], B * md * 6 * sizeof(float)));
        VC_TRY(host_alloc(e, (void**)&e->h_det_count2[k], B * sizeof(int)));
    }
    VC_TRY(host_alloc(e, (void**)&e->h_det, B * md * 6 * sizeof(float)));
    VC_TRY(host_alloc(e, (void**)&e->h_det_count, B * sizeof(int)));
    return VC_OK;
}

// C3(c1 -> c2, n x Bottleneck(e=1.0, shortcut), cv3 over concat(m(cv1 x), cv2 x)); models/common.py::C3
static View yolo_c3(PlanBuilder& pb, vc_engine* e, int idx, View x, View out, int cout, int reps, bool shortcut) {
    const std::string p = "model." + std::to_string(idx), bn = "c3_" + std::to_string(idx);
    const int h = cout / 2;
    auto& m = e->ybuf;
    View cat = mkview(m[bn + ".cat"], x.B, x.H, x.W, 2 * h, 0);
    View y = pb.conv(p + ".cv12", x, mkview(m[bn + ".a"], x.B, x.H, x.W, h, 0), 1, 1, 0, ACT_SILU);
    {   // channels [h, 2h) of the fused launch are C3.cv2 -> second half of the concat buffer
        ConvP& c = pb.ops->back().conv;
        View second = mkview(cat, x.B, x.H, x.W, h, h);
        c.out2 = second.ptr; c.out2_cs = second.cs; c.out2_co = second.co; c.split = h;
    }
    y.C = h;
    for (int j = 0; j < reps; ++j) {
        View t = pb.conv(p + ".m." + std::to_string(j) + ".cv1.conv", y, mkview(m[bn + ".t"], x.B, x.H, x.W, h, 0), 1, 1, 0, ACT_SILU);
        View dst = j == reps - 1 ? mkview(cat, x.B, x.H, x.W, h, 0) : mkview(m[bn + ((j % 2 == 0) ? ".b" : ".a")], x.B, x.H, x.W, h, 0);
        y = pb.conv(p + ".m." + std::to_string(j) + ".cv2.conv", t, dst, 3, 1, 1, ACT_SILU, shortcut ? &y : nullptr,
                    shortcut ? RES_AFTER_ACT : RES_NONE);
    }
    return pb.conv(p + ".cv3.conv", cat, out, 1, 1, 0, ACT_SILU);
}

// `sparse`: the sparse Detect head (yolo_forward decides; it is part of the plan's cache key).  A failed build leaves plan.ops empty.
int yolo_build_ops(vc_engine* e, int B, int Hn, int Wn, bool sparse, YoloPlan& plan) {
    std::vector<Op>& ops = plan.ops;
    plan.sparse = sparse;
    PlanBuilder pb{e, &e->yolo, &ops, e->prec};
    auto& m = e->ybuf;
    const int* c = e->ch;
    auto full = [&](const char* name, int stride, int C) { return mkview(m[name], B, Hn / stride, Wn / stride, C, 0); };
    View* lv = plan.layer_view;
    View x = full("in", 1, 4);
    lv[0] = x = pb.conv("model.0.conv", x, full("l0", 2, c[0]), 6, 2, 2, ACT_SILU);
    if (e->prec == PREC_FP8) {             // 3-channel stem in bf16 (K = 108), its output quantised once for the fp8 layers
        Op op{}; op.kind = Op::TO_FP8; op.a = x; op.b = full("l0q", 2, c[0]); op.b.B = x.B; op.b.H = x.H; op.b.W = x.W; ops.push_back(op);
        x = op.b;
    }
    lv[1] = x = pb.conv("model.1.conv", x, full("l1", 4, c[1]), 3, 2, 1, ACT_SILU);
    lv[2] = x = yolo_c3(pb, e, 2, x, full("l2", 4, c[1]), c[1], e->rep[0], true);
    lv[3] = x = pb.conv("model.3.conv", x, full("l3", 8, c[2]), 3, 2, 1, ACT_SILU);
    if (pb.status == VC_OK) ops.back().sole_reader_next = 1;      // "l3" is read by C3.cv1 | cv2 of layer 4 (the next op) and by nothing else
    View cat16 = full("cat16", 8, 2 * c[2]);
    lv[4] = x = yolo_c3(pb, e, 4, x, mkview(cat16, B, Hn / 8, Wn / 8, c[2], c[2]), c[2], e->rep[1], true);
    lv[5] = x = pb.conv("model.5.conv", x, full("l5", 16, c[3]), 3, 2, 1, ACT_SILU);
    if (pb.status == VC_OK) ops.back().sole_reader_next = 1;
    View cat12 = full("cat12", 16, 2 * c[3]);
    lv[6] = x = yolo_c3(pb, e, 6, x, mkview(cat12, B, Hn / 16, Wn / 16, c[3], c[3]), c[3], e->rep[2], true);
    lv[7] = x = pb.conv("model.7.conv", x, full("l7", 32, c[4]), 3, 2, 1, ACT_SILU);
    if (pb.status == VC_OK) ops.back().sole_reader_next = 1;
    lv[8] = x = yolo_c3(pb, e, 8, x, full("l8", 32, c[4]), c[4], e->rep[3], true);
    {   // SPPF (models/common.py::SPPF, k=5)
        View sc = full("sppcat", 32, 2 * c[4]);
        pb.conv("model.9.cv1.conv", x, mkview(sc, B, Hn / 32, Wn / 32, c[4] / 2, 0), 1, 1, 0, ACT_SILU);
        Op op{}; op.kind = Op::SPPF; op.a = sc; op.C = c[4] / 2; ops.push_back(op);
        lv[9] = x = pb.conv("model.9.cv2.conv", sc, full("l9", 32, c[4]), 1, 1, 0, ACT_SILU);
    }
    View cat22 = full("cat22", 32, 2 * c[3]);
    lv[10] = x = pb.conv("model.10.conv", x, mkview(cat22, B, Hn / 32, Wn / 32, c[3], c[3]), 1, 1, 0, ACT_SILU);
    { Op op{}; op.kind = Op::UPSAMPLE; op.a = x; op.b = mkview(cat12, B, Hn / 16, Wn / 16, c[3], 0); ops.push_back(op); lv[11] = op.b; }
    lv[12] = cat12;
    lv[13] = x = yolo_c3(pb, e, 13, cat12, full("l13", 16, c[3]), c[3], e->rep[0], false);
    View cat19 = full("cat19", 16, 2 * c[2]);
    lv[14] = x = pb.conv("model.14.conv", x, mkview(cat19, B, Hn / 16, Wn / 16, c[2], c[2]), 1, 1, 0, ACT_SILU);
    { Op op{}; op.kind = Op::UPSAMPLE; op.a = x; op.b = mkview(cat16, B, Hn / 8, Wn / 8, c[2], 0); ops.push_back(op); lv[15] = op.b; }
    lv[16] = cat16;
    // Detect.m[i]: 1x1 conv + bias (models/yolo.py::Detect).  fp32 mode: fp32 logits.  bf16 mode: bf16 logits like every other
    // activation, and the launch covers round_up(no, 8) output channels (the packed weight / bias rows past `no` are zero) so
    // that the 255-channel head takes the 16-byte-store epilogue; FLOPs are still counted for `no` channels (Op::cout_logical).
    const int no = 3 * (e->cfg.num_classes + 5), lcs = round_up(no, 8);
    // sparse Detect head (detect_post.hip): objectness conv over every pixel -> gather the pixels that can pass conf_thres -> the
    // full head on the gathered rows (row count on the device).  The work reported is what RUNS (the gathered rows); the dense
    // head's figures travel beside it as dense_* (round 3 credited the launch with the dense head's work: a 6 us launch showed
    // 3.4 x the chip's peak in the per-layer table).  The ops of level i follow the layer that produces its map: P3's and P4's are
    // marked Op::side and run on the head stream beside layers 18 - 23 (three short dependent launches per level, 0.11 ms of
    // objectness conv alone at 80^2, that used to sit at the END of the detector's chain of ~63 dependent launches).
    auto sparse_head = [&](int i, const View& x) {
        if (!sparse || pb.status != VC_OK) return;
        const size_t first = ops.size();
        const std::string hp = "model.24.m." + std::to_string(i);
        const double es = 2.0, Mh = (double)x.B * x.H * x.W;
        View ov{}; ov.ptr = e->d_obj[i]; ov.cs = 8; ov.co = 0;
        pb.conv(hp + ".obj", x, ov, 1, 1, 0, ACT_NONE);
        if (pb.status != VC_OK) return;
        ops.back().flops_override = 2.0 * Mh * 3 * x.C;                                    // the three objectness rows (the launch covers 8 zero-padded channels)
        ops.back().bytes_override = (Mh * x.C + 8.0 * x.C) * es + Mh * 8 * es;
        ops.back().dense_flops = 0; ops.back().dense_bytes = 0;                            // the dense head has no such launch: its work is on the head conv below
        { Op op{}; op.kind = Op::HEAD_COMPACT; op.level = i; op.a = x; ops.push_back(op); }
        View gx{}; gx.ptr = e->d_hc_x[i]; gx.B = 1; gx.H = 1; gx.W = e->hc_cap[i]; gx.C = x.C; gx.cs = x.C; gx.co = 0;
        View go{}; go.ptr = e->d_hc_logits[i]; go.cs = lcs; go.co = 0;
        pb.conv(hp, gx, go, 1, 1, 0, ACT_NONE);
        if (pb.status != VC_OK) return;
        Op& hop = ops.back();
        hop.cout_logical = hop.conv.Cout; hop.conv.Cout = lcs;
        hop.conv.m_dev = e->d_hc_count + i;
        // executed: the head on the gathered rows only (row count on the device, read back after the pass)
        hop.rows_level = i;
        hop.flops_override = 0; hop.bytes_override = (double)no * x.C * es;                // weights
        hop.flops_per_row = 2.0 * no * x.C; hop.bytes_per_row = (x.C + (double)lcs) * es;  // one gathered feature row in, one logit row out
        hop.dense_flops = 2.0 * Mh * no * x.C;
        hop.dense_bytes = (Mh * x.C + (double)no * x.C) * es + Mh * lcs * es;              // the dense head's in + weights + out
        if (i < 2) for (size_t j = first; j < ops.size(); ++j) ops[j].side = 1;
    };
    View p3 = lv[17] = yolo_c3(pb, e, 17, cat16, full("l17", 8, c[2]), c[2], e->rep[0], false);
    sparse_head(0, p3);
    lv[18] = pb.conv("model.18.conv", p3, mkview(cat19, B, Hn / 16, Wn / 16, c[2], 0), 3, 2, 1, ACT_SILU);
    lv[19] = cat19;
    View p4 = lv[20] = yolo_c3(pb, e, 20, cat19, full("l20", 16, c[3]), c[3], e->rep[0], false);
    sparse_head(1, p4);
    lv[21] = pb.conv("model.21.conv", p4, mkview(cat22, B, Hn / 32, Wn / 32, c[3], 0), 3, 2, 1, ACT_SILU);
    lv[22] = cat22;
    View p5 = lv[23] = yolo_c3(pb, e, 23, cat22, full("l23", 32, c[4]), c[4], e->rep[0], false);
    sparse_head(2, p5);
    const View heads[3] = {p3, p4, p5};
    for (int i = 0; i < 3 && !sparse; ++i) {
        View o{}; o.ptr = e->d_logits[i]; o.cs = lcs; o.co = 0;
        const bool wide = e->prec == PREC_F32;
        pb.conv("model.24.m." + std::to_string(i), heads[i], o, 1, 1, 0, ACT_NONE, nullptr, RES_NONE, wide);
        if (!wide && pb.status == VC_OK) { Op& op = ops.back(); op.cout_logical = op.conv.Cout; op.conv.Cout = lcs; }
        if (e->prec == PREC_FP8 && pb.status == VC_OK) ops.back().conv.out_bf16 = 1;        // logits leave the fp8 domain as bf16
    }
    if (pb.status != VC_OK) ops.clear();
    return pb.status;
}

// ------------------------------------------------------------------------------------------------ ReID net
static const struct { const char* name; int cin, cout; bool down; } kReidBlocks[8] = {
    {"layer1.0", 64, 64, false}, {"layer1.1", 64, 64, false}, {"layer2.0", 64, 128, true}, {"layer2.1", 128, 128, false},
    {"layer3.0", 128, 256, true}, {"layer3.1", 256, 256, false}, {"layer4.0", 256, 512, true}, {"layer4.1", 512, 512, false}};

void reid_define(vc_engine* e) {
    Net& n = e->reid;
    n.add("conv", 64, 3, 3, 3);
    for (const auto& b : kReidBlocks) {
        n.add(std::string(b.name) + ".conv1", b.cout, b.cin, 3, 3);
        n.add(std::string(b.name) + ".conv2", b.cout, b.cout, 3, 3);
        if (b.down || b.cin != b.cout) n.add(std::string(b.name) + ".downsample", b.cout, b.cin, 1, 1);
    }
}

int reid_cpad(int prec) { return prec == PREC_F32 ? 4 : 8; }

int reid_alloc(vc_engine* e) {
    const int es = elem_size(e->aux_prec);
    const size_t K = e->cfg.max_crops;
    auto& m = e->rbuf;
    VC_TRY(alloc_buf(e, m, "in", K * 50 * 50, reid_cpad(e->aux_prec), es));
    VC_TRY(alloc_buf(e, m, "r0", K * 50 * 50, 64, es));
    VC_TRY(alloc_buf(e, m, "x0", K * 25 * 25, 64, es));
    int hw = 25;
    for (int i = 0; i < 8; ++i) {
        const auto& b = kReidBlocks[i];
        if (b.down) hw = (hw - 1) / 2 + 1;
        const std::string p = b.name;
        VC_TRY(alloc_buf(e, m, p + ".t", K * hw * hw, b.cout, es));
        VC_TRY(alloc_buf(e, m, p + ".y", K * hw * hw, b.cout, es));
        if (b.down || b.cin != b.cout) VC_TRY(alloc_buf(e, m, p + ".d", K * hw * hw, b.cout, es));
    }
    VC_TRY(dev_alloc(e, (void**)&e->d_crops, K * 5 * sizeof(int)));
    VC_TRY(host_alloc(e, (void**)&e->h_crops, K * 5 * sizeof(int)));
    VC_TRY(dev_alloc(e, (void**)&e->d_feat, K * VC_FEAT_DIM * sizeof(float)));
    for (int q = 0; q < 3; ++q) {                      // stream path: ReID of batches i+1 / i+2 runs while batch i is tracked
        VC_TRY(dev_alloc(e, (void**)&e->d_feat2[q], K * VC_FEAT_DIM * sizeof(float)));
        VC_TRY(dev_alloc(e, (void**)&e->d_crops2[q], K * 5 * sizeof(int)));
        VC_TRY(host_alloc(e, (void**)&e->h_crops2[q], K * 5 * sizeof(int)));
    }
    VC_TRY(host_alloc(e, (void**)&e->h_feat, K * VC_FEAT_DIM * sizeof(float)));
    VC_TRY(dev_alloc(e, (void**)&e->d_reid_in_nchw, K * 3 * 50 * 50 * sizeof(float)));
    return VC_OK;
}

// the op plan of crops [k0, k0 + k) of the "in" buffer (empty if the build fails); plan.out is what the average pool reads
int reid_build_ops(vc_engine* e, int k0, int k, ReidPlan& plan) {
    std::vector<Op>& ops = plan.ops;
    PlanBuilder pb{e, &e->reid, &ops, e->aux_prec};
    auto& m = e->rbuf;
    View x = mkview(m["in"], k, 50, 50, reid_cpad(e->aux_prec), 0);
    x.ptr = (char*)x.ptr + (size_t)k0 * 50 * 50 * reid_cpad(e->aux_prec) * elem_size(e->aux_prec);
    x = pb.conv("conv", x, mkview(m["r0"], k, 50, 50, 64, 0), 3, 1, 1, ACT_RELU);             // model.py:51-55
    { Op op{}; op.kind = Op::MAXPOOL; op.a = x; op.b = mkview(m["x0"], k, 25, 25, 64, 0); ops.push_back(op); x = op.b; }   // :58
    for (const auto& b : kReidBlocks) {                                                        // BasicBlock.forward, model.py:30-38
        const std::string p = b.name;
        const int s = b.down ? 2 : 1;
        View t = pb.conv(p + ".conv1", x, mkview(m[p + ".t"], k, 0, 0, b.cout, 0), 3, s, 1, ACT_RELU);
        View sc = x;
        if (b.down || b.cin != b.cout) sc = pb.conv(p + ".downsample", x, mkview(m[p + ".d"], k, 0, 0, b.cout, 0), 1, s, 0, ACT_NONE);
        x = pb.conv(p + ".conv2", t, mkview(m[p + ".y"], k, 0, 0, b.cout, 0), 3, 1, 1, ACT_RELU, &sc, RES_BEFORE_ACT);
    }
    plan.out = x;
    if (pb.status != VC_OK) ops.clear();
    return pb.status;
}

}  // namespace vc
