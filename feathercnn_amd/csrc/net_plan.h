// net_plan.h -- what runs between LoadWeights and the launches: the collapse passes and fuse_layers (once), plan_chains / plan_siblings /
// plan_concurrency (after every Reshape), reshape_all, prepare, run_layers and forward.
#pragma once
#include "net_detect.h"
#include "wino_gemm_policy.h" // FHIP_M_NT_BYTES: the size class of M the colpass rule shares with the tile GEMM's store policy

namespace fhip::net
{

static bool is_channel_map_type(const Layer* l)
{
    // a layer typed "Concat" need not be a ConcatLayer (the collapsed detection head of net_detect.h keeps the type string): ask the object
    const ConcatLayer* cat = l->type == "Concat" ? dynamic_cast<const ConcatLayer*>(l) : nullptr;
    return l->type == "ShuffleChannel" || l->type == "Slice" || (cat && cat->axis == 0);
}

// Fusion level 2: a run of Concat / ShuffleChannel / Slice layers, in any order, that follow each other in the layer list and are linked
// by blobs with exactly one consumer becomes one ChannelMapLayer (ShuffleNet v2's Concat -> ShuffleChannel -> Slice: two bottoms, two
// tops, one launch).  The layer keeps the type and name of the run's first layer; the linking blobs are fused away.  A run of Concat
// layers alone is left as it is (their copies are not this route's); a run with more bottoms or tops than one map takes is cut
// back to its longest prefix that fits.
static void collapse_channel_maps(Net& net)
{
    auto holds = [](const std::vector<Blob*>& v, const Blob* b) { return std::find(v.begin(), v.end(), b) != v.end(); };
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        if (!is_channel_map_type(net.layers[i].get())) continue;
        std::vector<Blob*> made = net.layers[i]->tops;
        size_t end = i + 1;
        for (; end < net.layers.size(); ++end)
        {
            const Layer* l = net.layers[end].get();
            if (!is_channel_map_type(l)) break;
            bool reads = false, sole = true;
            for (const Blob* b : l->bottoms)
                if (holds(made, b))
                {
                    reads = true;
                    sole = sole && readers(net, b).count == 1;
                }
            if (!reads || !sole) break;
            made.insert(made.end(), l->tops.begin(), l->tops.end());
        }
        // the longest prefix of the run that moves channels and fits one map
        std::vector<Blob*> sources, inner, finals;
        for (; end - i >= 2; --end)
        {
            sources.clear();
            inner.clear();
            finals.clear();
            bool moves = false;
            for (size_t k = i; k < end; ++k)
            {
                moves = moves || net.layers[k]->type != "Concat";
                for (Blob* b : net.layers[k]->bottoms)
                {
                    if (holds(made, b))
                        inner.push_back(b);
                    else if (!holds(sources, b))
                        sources.push_back(b);
                }
            }
            for (size_t k = i; k < end; ++k)
                for (Blob* t : net.layers[k]->tops)
                    if (!holds(inner, t)) finals.push_back(t);
            if (moves && sources.size() <= FHIP_CHANNEL_MAP_MAX_BLOBS && finals.size() <= FHIP_CHANNEL_MAP_MAX_BLOBS) break;
        }
        if (end - i < 2) continue;
        std::unique_ptr<ChannelMapLayer> run(new ChannelMapLayer);
        run->type = net.layers[i]->type;
        run->name = net.layers[i]->name;
        run->net = &net;
        run->bottoms = sources;
        run->tops = finals;
        for (size_t k = i; k < end; ++k)
        {
            Layer* l = net.layers[k].get();
            if (l->type == "Concat")
            {
                MapStep st;
                st.kind = MapStep::CONCAT;
                st.name = l->name;
                st.bottoms = l->bottoms;
                st.tops = l->tops;
                run->steps.push_back(st);
            }
            else
                run->steps.push_back(static_cast<ChannelMapLayer*>(l)->steps[0]);
        }
        for (Blob* b : inner) b->fused_away = true;
        net.layers[i] = std::move(run);
        net.layers.erase(net.layers.begin() + i + 1, net.layers.begin() + end);
    }
}

static bool sum_tail(const Net& net, Blob* b, int sum, SumTail& t)
{
    if (sum < 0) return false;
    const Layer* l = net.layers[sum].get();
    const EltwiseLayer* elt = net.layers[sum]->as_eltwise(); // LoadParam took SUM without coefficients only
    if (!elt || l->bottoms.size() != 2 || l->tops.size() != 1 || l->bottoms[0] == l->bottoms[1]) return false;
    t = SumTail();
    t.other = l->bottoms[0] == b ? l->bottoms[1] : l->bottoms[0];
    t.sum = t.last = sum;
    t.sum_top = t.top = l->tops[0];
    t.inner.assign(1, b);
    t.relu = elt->relu;
    if (t.relu) return true;
    const int j = readers(net, t.top).sole(); // behind the sum where there is one: a reader never precedes its producer (see readers)
    if (j > sum && net.layers[j]->bottoms.size() == 1 && net.layers[j]->tops.size() == 1 && is_plain_relu(net.layers[j].get()))
    {
        t.relu = true;
        t.relu_layer = t.last = j;
        t.inner.push_back(t.top);
        t.top = net.layers[j]->tops[0];
    }
    return true;
}

// Fusion level 2: a squeeze-and-excitation block,
//
//   Split(x) -> Pooling(global, average) -> {InnerProduct | Convolution 1x1, group 1} -> [ReLU | Swish]
//            -> {InnerProduct | Convolution 1x1, group 1} -> {Sigmoid | HardSigmoid}
//            -> {BinaryOp mul | Scale -233}(x, gate)   [-> Eltwise SUM with another blob [-> plain ReLU]]
//
// where every linking blob has exactly one consumer, becomes one GateBlockLayer.  The pass runs BEFORE the pairwise Fuse pass of
// fuse_layers: afterwards the first excite layer would already have absorbed its ReLU and the block would no longer read as written.
// The layer keeps the Pooling layer's type and name and takes the place of the block's LAST layer in the list: the shortcut of a residual
// block may be produced between the Pooling layer and the Eltwise layer, and everything the block reads is ready where its last layer
// stood.  A block that does not match (a linking blob with a second consumer, a grouped, strided or padded excite convolution, a pooling
// that is not global average, operands that are not two tops of one Split) stays layer by layer.
static void collapse_gate_blocks(Net& net)
{
    auto one_to_one = [](const Layer* l) { return l->bottoms.size() == 1 && l->tops.size() == 1; };
    // W [out][in] and bias of an InnerProduct or of a plain 1x1 convolution
    auto dense = [&](Layer* l, int& in, int& out, std::vector<float>& w, std::vector<float>& b, bool& has_b) {
        if (!one_to_one(l)) return false;
        if (l->type == "InnerProduct")
        {
            InnerProductLayer* ip = static_cast<InnerProductLayer*>(l);
            if (ip->quant || ip->p.activation != FHIP_ACT_NONE || ip->w_host.size() != ip->input_size * ip->output_size) return false;
            in = (int)ip->input_size, out = (int)ip->output_size, w = ip->w_host, b = ip->b_host, has_b = ip->p.bias_term != 0;
            return true;
        }
        if (l->type != "Convolution") return false; // not "ConvolutionDepthWise": kept as found (the group test below turns a real one away)
        ConvLayer* cv = l->as_conv();
        const fhip_conv_param& p = cv->p;
        if (cv->route != ROUTE_MAIN || p.group != 1 || p.kernel_h != 1 || p.kernel_w != 1 || p.stride_h != 1 || p.stride_w != 1 || p.pad_left || p.pad_right ||
            p.pad_top || p.pad_bottom || p.activation != FHIP_ACT_NONE || !cv->fold.empty() || cv->w_host.size() != (size_t)p.input_channels * p.output_channels)
            return false;
        in = p.input_channels, out = p.output_channels, w = cv->w_host, b = cv->b_host, has_b = p.bias_term != 0;
        return true;
    };
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        Layer* pool = net.layers[i].get();
        if (!pool->as_pooling() || !one_to_one(pool)) continue;
        const fhip_pool_param& q = pool->as_pooling()->q;
        if (!q.global_pooling || q.pooling_type == 0) continue;
        std::vector<int> gone(1, (int)i);
        std::vector<Blob*> inner;
        std::unique_ptr<GateBlockLayer> blk(new GateBlockLayer);
        auto step = [&](Blob* top) -> Layer* { // the layer behind a linking blob
            const int j = readers(net, top).sole();
            if (j < 0) return nullptr;
            gone.push_back(j);
            inner.push_back(top);
            return net.layers[j].get();
        };
        Layer* l = step(pool->tops[0]);
        int in2 = 0, out2 = 0;
        if (!l || !dense(l, blk->C, blk->R, blk->w1, blk->b1, blk->has_b1)) continue;
        if (!(l = step(l->tops[0]))) continue;
        if (one_to_one(l) && (is_plain_relu(l) || l->type == "Swish"))
        {
            blk->mact = l->type == "Swish" ? FHIP_EXCITE_MACT_SWISH : FHIP_EXCITE_MACT_RELU;
            if (!(l = step(l->tops[0]))) continue;
        }
        if (!dense(l, in2, out2, blk->w2, blk->b2, blk->has_b2) || in2 != blk->R || out2 != blk->C) continue;
        if (!(l = step(l->tops[0])) || !one_to_one(l)) continue;
        if (l->type == "HardSigmoid")
        {
            blk->gact = FHIP_EXCITE_GACT_HARDSIGMOID;
            blk->alpha = static_cast<GateActivationLayer*>(l)->alpha;
            blk->beta = static_cast<GateActivationLayer*>(l)->beta;
        }
        else if (l->type != "Sigmoid")
            continue;
        Blob* g = l->tops[0];
        if (!(l = step(g)) || l->bottoms.size() != 2 || l->tops.size() != 1) continue;
        Blob* x = nullptr;
        if (l->type == "BinaryOp" && static_cast<BinaryOpLayer*>(l)->multiplies())
            x = l->bottoms[0] == g ? l->bottoms[1] : l->bottoms[0];
        else if (l->type == "BinaryOp")
            continue; // an add, sub, div, max or min behind the gate's activation is no gate
        else if (l->type == "Scale" && static_cast<ScaleLayer*>(l)->gated && l->bottoms[1] == g)
            x = l->bottoms[0];
        if (!x || x == g || x == pool->bottoms[0]) continue;
        bool siblings = false; // the squeezed and the gated blob are two tops of one Split: the same tensor
        for (auto& s : net.layers)
            if (s->type == "Split")
            {
                bool a = false, b = false;
                for (const Blob* t : s->tops) a = a || t == pool->bottoms[0], b = b || t == x;
                siblings = siblings || (a && b);
            }
        if (!siblings) continue;
        blk->bottoms.push_back(pool->bottoms[0]);
        blk->bottoms.push_back(x);
        Blob* out = l->tops[0];
        SumTail tail;
        if (sum_tail(net, out, readers(net, out).sole(), tail))
        {
            blk->bottoms.push_back(tail.other);
            gone.push_back(tail.sum);
            if (tail.relu_layer >= 0) gone.push_back(tail.relu_layer);
            inner.insert(inner.end(), tail.inner.begin(), tail.inner.end());
            if (tail.relu) blk->act = FHIP_GATE_ACT_RELU;
            out = tail.top;
        }
        bool forward = true; // the chain runs down the list
        for (size_t k = 1; k < gone.size(); ++k) forward = forward && gone[k] > gone[k - 1];
        if (!forward) continue;
        blk->type = pool->type;
        blk->name = pool->name;
        blk->net = &net;
        blk->q = q;
        blk->tops.assign(1, out);
        for (Blob* b : inner) b->fused_away = true;
        for (int j : gone) blk->parts.push_back(std::move(net.layers[j])); // kept for the shapes that run stepwise
        net.layers[gone.back()] = std::move(blk);
        for (size_t k = gone.size() - 1; k-- > 0;) net.layers.erase(net.layers.begin() + gone[k]);
        --i; // the layer that moved into slot i has not been looked at
    }
}

// Fusion level 2: FPN's upsample-and-add,
//
//   Interp(x [, size]) -> Eltwise SUM (two bottoms, no coefficients) with another blob [-> plain ReLU]
//
// where the Interp's top -- and the sum's, if a ReLU follows -- has exactly one consumer, becomes the InterpLayer alone: the other operand is
// its last bottom (residual_at) and the whole chain is one launch that never writes the up-sampled tensor.  Like collapse_gate_blocks the
// pass runs before the pairwise Fuse pass and the layer takes the place of the chain's LAST layer in the list: the other operand (FPN's
// lateral convolution) may be produced between the Interp and the Eltwise layer.  The layer keeps its type and name; the blobs inside the
// chain refuse Extract.  An Interp whose top has a second consumer stays as written.
static void collapse_upsample_adds(Net& net)
{
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        InterpLayer* up = net.layers[i]->as_interp();
        if (!up || up->residual_at >= 0 || up->tops.size() != 1) continue;
        const int jsum = readers(net, up->tops[0]).sole();
        SumTail tail;
        if (jsum <= (int)i || !sum_tail(net, up->tops[0], jsum, tail)) continue;
        up->bottoms.push_back(tail.other);
        up->residual_at = (int)up->bottoms.size() - 1;
        up->relu = tail.relu;
        up->tops[0] = tail.top;
        for (Blob* b : tail.inner) b->fused_away = true;
        std::unique_ptr<Layer> moved = std::move(net.layers[i]);
        net.layers[tail.last] = std::move(moved); // the ReLU (or the Eltwise) is dropped, the Interp stands in its place
        if (tail.last != jsum) net.layers.erase(net.layers.begin() + jsum);
        net.layers.erase(net.layers.begin() + i);
        --i; // the layer that moved into slot i has not been looked at
    }
}

// Fusion level >= 2, in a net with fhip_net_set_frame: a Padding layer that only zero-pads the plane (type 0, value 0, no per-channel
// values, no channel margins: Layer::zero_pad_margins) and whose top is read by exactly one Convolution / ConvolutionDepthWise on the main
// or the grouped fp32 route with pads >= 0 (ConvLayer::FoldPadding) is removed: the convolution reads the Padding's bottom with the margins
// added to its own four pads, and the blob between them refuses Extract.  This is what a converter writes in front of TensorFlow's
// stride-2 "SAME" convolutions (0, 1, 0, 1), where the Padding is a copy of the whole tensor that buys nothing.  Runs before every other
// pass, so the algorithm and every later fusion are chosen on the folded parameters.
static void fold_zero_paddings(Net& net)
{
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        Layer* pad = net.layers[i].get();
        const int* margins = pad->zero_pad_margins();
        if (!margins || pad->tops.size() != 1 || pad->bottoms.size() != 1) continue;
        const int reader = readers(net, pad->tops[0], i + 1).sole();
        if (reader < 0) continue;
        ConvLayer* conv = net.layers[reader]->as_conv();
        if (!conv || conv->bottoms.size() != 1 || !conv->FoldPadding(margins)) continue;
        conv->bottoms[0] = pad->bottoms[0];
        pad->tops[0]->fused_away = true;
        net.layers.erase(net.layers.begin() + i);
        --i;
    }
}

// The fusion pass of layer.cpp:82-101 (TryFuse): a layer absorbs the single consumer of its single top.
static void fuse_layers(Net& net)
{
    if (net.fused) return;
    net.fused = true;
    if (net.fusion <= 0) return;
    if (net.fusion >= 2) fold_zero_paddings(net);
    if (net.fusion >= 2) collapse_detection_heads(net);
    if (net.fusion >= 2) collapse_channel_maps(net);
    if (net.fusion >= 2) collapse_gate_blocks(net);
    if (net.fusion >= 2) collapse_upsample_adds(net);
    if (net.fusion >= 2 && net.transformer) collapse_add_norms(net);
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        for (;;)
        {
            Layer* cur = net.layers[i].get();
            if (cur->tops.size() != 1) break;
            Blob* top = cur->tops[0];
            const int consumer = readers(net, top, i + 1).sole();
            if (consumer < 0) break;
            Layer* nx = net.layers[consumer].get();
            SumTail tail;
            if (net.fusion >= 2 && cur->as_conv() && sum_tail(net, top, consumer, tail))
            {
                // conv -> Eltwise(sum with an EARLIER blob) [-> ReLU]: the add moves into the conv's epilogue; the ReLU layer, where the
                // tail has one, is absorbed like any other by the next round (ConvLayer::Fuse)
                bool earlier = false;
                for (size_t j = 0; j < i; ++j)
                    for (Blob* t : net.layers[j]->tops) earlier = earlier || t == tail.other;
                if (!earlier || !cur->as_conv()->FuseResidual(tail.other)) break;
                top->fused_away = true;
                cur->tops[0] = tail.sum_top;
                net.layers.erase(net.layers.begin() + consumer);
                continue;
            }
            if (nx->bottoms.size() != 1 || nx->tops.size() != 1) break;
            const int fr = cur->Fuse(nx, net.fusion);
            if (fr != 1 && fr != 2) break;
            if (fr == 2) cur->as_conv()->ep.pw.reset(net.layers[consumer].release()->as_conv()); // adopted, not dropped
            top->fused_away = true;
            cur->tops[0] = nx->tops[0];
            net.layers.erase(net.layers.begin() + consumer);
        }
    }
}

// Which layers may leave the main stream (see Net::concurrency).  Needs the algorithms chosen by Reshape: only layers without
// scratch (the arena is shared) qualify.
static int plan_concurrency(Net& net)
{
    const size_t L = net.layers.size();
    net.side.assign(L, -1);
    net.waits.assign(L, std::vector<int>());
    if (!net.concurrency) return 0;
    int pairs = 0;
    for (size_t i = 0; i < L; ++i)
    {
        Layer* l = net.layers[i].get();
        if (!l->as_conv() || l->arena_bytes() != 0 || l->tops.size() != 1) continue;
        if (l->sibling_state()) continue; // writes (or is written with) the top of its neighbour: stays on the net's stream
        const int sole = readers(net, l->tops[0], i + 1, true).sole();
        if (sole <= (int)i + 1) continue; // none, several, or the very next layer
        const size_t consumer = (size_t)sole;
        bool work_between = false; // something worth overlapping with
        for (size_t j = i + 1; j < consumer; ++j) work_between = work_between || net.layers[j]->algo() >= 0;
        if (!work_between) continue;
        net.side[i] = pairs;
        net.waits[consumer].push_back(pairs);
        ++pairs;
    }
    if (pairs && !net.side_stream) FHIP_CHECK_HIP(hipStreamCreateWithFlags(&net.side_stream, hipStreamNonBlocking));
    while (net.events.size() < (size_t)2 * pairs)
    {
        hipEvent_t e;
        FHIP_CHECK_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        net.events.push_back(e);
    }
    return 0;
}

// Fusion level 3, after Reshape (needs the routes and shapes): a Winograd layer directly followed by the 3x3 / stride-1 / pad-1 Winograd
// layer that is the only consumer of its top hands over its output already transformed (fhip_conv_forward_chained); the blob between
// them gets no storage.  VGG-16: conv1_2 ... conv5_3 become one run.
static int plan_chains(Net& net)
{
    const size_t L = net.layers.size();
    std::vector<ConvLayer*> conv(L, nullptr);
    for (size_t i = 0; i < L; ++i)
        if ((conv[i] = net.layers[i]->as_conv())) conv[i]->chain.reset();
    for (auto& kv : net.blobs) kv.second->chained = false;
    for (auto& b : net.shadowed) b->chained = false; // blobs whose name a later top re-used (in-place style .param files) re-plan too
    net.chain_slot[0] = net.chain_slot[1] = net.chain_m = 0;
    if (net.fusion < 3) return 0;
    // A layer of a run, or the consumer of a first layer.  Of the claims only the pair and the residual turn a layer away: a pooled boundary
    // may be chained, the chain and head marks are this pass's own and being written (the scans below test the ones they mean), and the
    // sibling plan is still the previous shape's -- plan_siblings runs behind this pass.
    auto plain = [](const ConvLayer* c) {
        return c && c->unclaimed(CLAIM_POOL | CLAIM_CHAIN | CLAIM_HEAD | CLAIM_SIBLING) && c->algo_ == FHIP_WINOGRADF63 && c->tops.size() == 1 && c->bottoms.size() == 1;
    };
    auto chain_away = [](Blob* b) {
        b->chained = true;
        b->drop_storage();
    };
    for (size_t i = 0; i + 1 < L; ++i)
    {
        ConvLayer *a = conv[i], *b = conv[i + 1];
        if (!plain(a) || !plain(b) || b->bottoms[0] != a->tops[0]) continue;
        if (a->ep.fuse_pool && !a->ep.pool_fast) continue;
        if (readers(net, a->tops[0], 0, true).count != 1) continue;
        if (!fhip_conv_can_chain_winograd(&a->p, a->algo_, &b->p, b->algo_, a->ep.fuse_pool ? 1 : 0)) continue;
        ChainPlan::link(a, b);
        chain_away(a->tops[0]);
    }
    // 2x2 image canvases (feather_canvas.h): a maximal sub-run of chained layers on one plane size, entered through a pooled boundary, whose
    // planes are whole tiles as canvases (14 and 56 pixels: 0.69 x and 0.90 x the tiles) runs with four images of a channel per "image".
    // It ends in a pooled boundary to a plain layer, or with the run (the canvas output transform; a pooling that is not fused stays plain).
    for (size_t i = 0; i < L; ++i)
    {
        ConvLayer* c = conv[i];
        if (!c || !c->chain.in || c->chain.canvas) continue;
        ConvLayer* prev = nullptr;
        for (size_t j = 0; j < i; ++j)
            if (conv[j] && conv[j]->chain.next == c) prev = conv[j];
        if (!prev || prev->chain.canvas || !prev->ep.fuse_pool || prev->chain.head) continue; // a sub-run starts behind a plain layer's pooled boundary
        const int n = c->bottoms[0]->n;
        fhip_conv_param q;
        if (fhip_winograd_f63_canvas_param(&prev->p, n, &q) == FHIP_OK) continue; // (never: a pooled consumer of a canvas plane is not one)
        if (prev->p.kernel_h != 3 || prev->p.pad_left != 1 || prev->p.pad_right != 1 || prev->p.pad_top != 1 || prev->p.pad_bottom != 1 ||
            prev->p.output_h != prev->p.output_w || prev->p.output_h != prev->p.input_h)
            continue;
        std::vector<ConvLayer*> run;
        for (ConvLayer* x = c; x; x = x->chain.next)
        {
            if (x->p.input_h != c->p.input_h || x->p.input_w != c->p.input_w || fhip_winograd_f63_canvas_param(&x->p, n, &q) != FHIP_OK) break;
            if (x->p.activation != FHIP_ACT_NONE && x->p.activation != FHIP_ACT_RELU) break;
            run.push_back(x);
            if (x->ep.fuse_pool) break; // the plane size changes behind it
        }
        if (run.empty()) continue;
        ConvLayer* last = run.back();
        // the sub-run must be the whole stretch on this plane size, and leave through a form that exists: EXIT (pooled), or the end of the run
        if (last->chain.next && !last->ep.fuse_pool) continue;
        if (!last->chain.next && last->ep.fuse_pool && !last->ep.pool_fast) continue;
        if (!canvas_api()) return FHIP_E_UNSUPPORTED; // message set by canvas_api
        for (ConvLayer* x : run) x->chain.to_canvas(x->p, n);
    }
    // a first layer in front of a Winograd layer (VGG-16: conv1_1 -> conv1_2) is computed inside that layer's input transform
    for (size_t i = 0; i + 1 < L; ++i)
    {
        ConvLayer *a = conv[i], *b = conv[i + 1];
        // on the main library (a grouped layer is no first_candidate) and unclaimed -- but for the head marks, which this scan never looked
        // at, and the sibling plan, which is the previous shape's here
        if (!a || a->route != ROUTE_MAIN || !a->unclaimed(CLAIM_HEAD | CLAIM_SIBLING) || a->tops.size() != 1 || a->bottoms.size() != 1) continue;
        if (!a->first_candidate() || !plain(b) || b->chain.in || b->bottoms[0] != a->tops[0]) continue;
        if (readers(net, a->tops[0], 0, true).count != 1) continue;
        if (!fhip_conv_can_fuse_first_winograd(&a->p, &b->p, b->algo_, a->bottoms[0]->n)) continue;
        ChainPlan::absorb_first(a, b);
        chain_away(a->tops[0]);
    }
    // blobs the previous plan had chained and this one did not: Reshape left them without storage
    auto restore = [](Blob* b) -> int {
        if (b->chained || b->data || b->alias || b->fused_away || b->count() == 0) return 0;
        FHIP_CHECK_HIP(hipMalloc((void**)&b->data, b->count() * sizeof(float)));
        b->capacity = b->count();
        return 0;
    };
    for (auto& kv : net.blobs)
        if (const int rc = restore(kv.second.get())) return rc;
    for (auto& b : net.shadowed)
        if (const int rc = restore(b.get())) return rc;
    auto up = [](size_t x) { return (x + 255) / 256 * 256; };
    size_t slot[2] = {0, 0}, msz = 0;
    for (ConvLayer* c : conv)
    {
        if (!c || !c->chain.runs()) continue;
        const int rc = c->chain.plan_run(c->p, c->bottoms[0]->n);
        if (rc) return rc;
        slot[c->chain.pos & 1] = std::max(slot[c->chain.pos & 1], up(c->chain.run_plan.v_bytes));
        msz = std::max(msz, up(c->chain.run_plan.m_bytes));
    }
    // The column-passed tile GEMM (feather_colpass.h, fhip_net_set_colpass): a chained layer the library accepts, followed by a plain chained
    // layer, neither on canvases.  Mode 1 takes it where M is of the size class in which GEMM and boundary are HBM-bound (FHIP_M_NT_BYTES,
    // csrc/wino_gemm_policy.h: VGG-16 b32's conv1_2 and conv2_1) and keeps the main route in a tree without the library; mode 2 takes it
    // wherever accepted and needs the library.  M48 fits the M slot sized above.
    if (net.colpass)
        for (ConvLayer* c : conv)
        {
            if (!c || !c->chain.next || c->chain.canvas || c->chain.next->chain.canvas) continue;
            if (net.colpass == 1 && c->chain.run_plan.m_bytes < (size_t)FHIP_M_NT_BYTES) continue;
            // the library's rule, stated here too so that a net it would refuse anyway never opens it
            const fhip_conv_param& q = c->p;
            if (q.input_channels != 64 || q.output_channels < 64 || (q.output_channels & 63) || c->chain.run_plan.frequency_points != 64) continue;
            if (q.activation != FHIP_ACT_NONE && q.activation != FHIP_ACT_RELU) continue;
            const ColpassApi* api = net.colpass == 2 ? colpass_api() : colpass_api_quiet();
            if (!api && net.colpass == 2) return FHIP_E_UNSUPPORTED; // message set by colpass_api
            if (!api) break;
            c->chain.colpass = api->supported(&q, c->bottoms[0]->n) == FHIP_OK;
        }
    net.chain_slot[0] = 0;
    net.chain_slot[1] = slot[0];
    net.chain_m = slot[0] + slot[1];
    for (ConvLayer* c : conv)
        if (c && c->chain.runs()) c->chain.arena(slot[0] + slot[1] + msz);
    return 0;
}

// Fusion level 2, after Reshape (needs routes, shapes and the batch): two 1x1 convolutions that follow each other in the layer list and
// read the same blob with the same stride run as one GEMM (fhip_conv_forward_siblings).  ResNet-50: res3a / res4a / res5a branch1 + branch2a.
static int plan_siblings(Net& net)
{
    const size_t L = net.layers.size();
    std::vector<ConvLayer*> conv(L, nullptr);
    // layers typed "Convolution" only: a "ConvolutionDepthWise" layer never becomes a sibling.  Kept as found -- the code gives no reason
    // (fhip_conv_can_fuse_siblings has its own tests of the geometry)
    for (size_t i = 0; i < L; ++i)
        if (net.layers[i]->type != "ConvolutionDepthWise" && (conv[i] = net.layers[i]->as_conv())) conv[i]->sibs.reset();
    if (net.fusion < 2) return 0;
    auto root = [](const Blob* b) { return b->alias ? b->alias : b; };
    auto plain = [](const ConvLayer* c) { return c && c->unclaimed() && c->algo_ == FHIP_IM2COL && c->tops.size() == 1 && c->bottoms.size() == 1; };
    auto pairs = [&](const ConvLayer* a, const ConvLayer* b) {
        if (!plain(a) || !plain(b) || root(a->bottoms[0]) != root(b->bottoms[0]) || a->tops[0] == b->tops[0]) return false;
        // both layers on the 128-row tile when alone (a 64-row layer -- ResNet's res2a_branch2a -- is faster on its own 64 x 128 tile:
        // tools/sibling_bench.py 116 vs 126 us for the pair)
        if (a->p.output_channels <= 64 || b->p.output_channels <= 64) return false;
        return fhip_conv_can_fuse_siblings(&a->p, a->algo_, &b->p, b->algo_, a->bottoms[0]->n) != 0;
    };
    // a layer's partner is the next one or none, so layer i's part of the plan is settled once this loop has looked at (i, i + 1)
    for (size_t i = 0; i < L; ++i)
    {
        if (i + 1 < L && pairs(conv[i], conv[i + 1]))
            SiblingPlan::pair(conv[i], conv[i + 1]);
        else if (conv[i])
            conv[i]->sibs.unpaired();
    }
    return 0;
}

// The layer a q8 blob's bytes come from: the requantised convolution above the ReLU, max Pooling and Split layers that pass them on.
static const Layer* q8_producer(Net& net, const Blob* b)
{
    Layer* found = nullptr;
    for (size_t hops = 0; hops <= net.layers.size(); ++hops)
    {
        Layer* writer = nullptr;
        for (auto& l : net.layers)
            for (const Blob* t : l->tops)
                if (t == b) writer = l.get();
        if (!writer) break;
        found = writer;
        if (writer->bottoms.empty() || !writer->bottoms[0]->q8 || writer->as_conv()) break;
        b = writer->bottoms[0];
    }
    return found;
}

static int reshape_all(Net& net)
{
    net.drop_graph();
    size_t need = 0;
    for (auto& l : net.layers)
    {
        // q8 blobs: a layer that cannot read one is refused; whether the layer's tops are q8 is settled before its Reshape sizes them
        for (const Blob* b : l->bottoms)
            if (b->q8 && !l->reads_q8())
            {
                const Layer* from = q8_producer(net, b);
                return failf(NET_E_TOPOLOGY, "blob %s holds the int8 output of layer %s, which %s layer %s cannot read", b->name.c_str(),
                             from ? from->name.c_str() : "?", l->type.c_str(), l->name.c_str());
            }
        const bool q8 = !l->bottoms.empty() && l->writes_q8();
        for (Blob* t : l->tops) t->q8 = q8;
        const int rc = l->Reshape();
        if (rc) return rc;
    }
    {
        int rc = plan_chains(net);
        if (rc) return rc;
        if ((rc = plan_siblings(net))) return rc;
    }
    for (auto& l : net.layers) need = std::max(need, l->arena_bytes());
    // one scratch arena shared by every layer = max over layers (mempool.cpp:88-92)
    if (need > net.arena.bytes)
    {
        const int rc = net.arena.resize(need);
        if (rc) return rc;
    }
    net.shapes_dirty = false;
    return plan_concurrency(net);
}

static int prepare(Net& net)
{
    if (!net.param_loaded) return failf(NET_E_IO, "Network has not been loaded. Please load the param file first.");
    if (!net.weights_loaded)
    {
        bool needs = false;
        for (auto& l : net.layers) needs = needs || l->needs_weights();
        if (needs) return failf(NET_E_IO, "weights have not been loaded");
    }
    fuse_layers(net);
    for (auto& kv : net.blobs)
        if (!kv.second->fused_away && kv.second->count() == 0)
        {
            bool is_input = false;
            for (auto& l : net.layers)
                if (l->type == "Input")
                    for (Blob* tb : l->tops) is_input = is_input || tb == kv.second.get();
            if (is_input) return failf(NET_E_SHAPE, "input blob %s has not been fed", kv.first.c_str());
        }
    if (net.shapes_dirty)
    {
        const int rc = reshape_all(net);
        if (rc) return rc;
    }
    for (auto& l : net.layers) // Init is a no-op for a layer whose packed weights are still valid
    {
        const int rc = l->Init(net.stream);
        if (rc) return rc;
    }
    net.initialized = true;
    return 0;
}

static int run_layers(Net& net)
{
    for (size_t i = 0; i < net.layers.size(); ++i)
    {
        Layer* l = net.layers[i].get();
        if (i < net.side.size() && net.side[i] >= 0)
        {
            hipEvent_t fork = net.events[2 * net.side[i]], join = net.events[2 * net.side[i] + 1];
            FHIP_CHECK_HIP(hipEventRecord(fork, net.stream)); // everything this layer reads is produced earlier on the main stream
            FHIP_CHECK_HIP(hipStreamWaitEvent(net.side_stream, fork, 0));
            const int rc = l->Forward(net.side_stream);
            if (rc) return rc;
            FHIP_CHECK_HIP(hipEventRecord(join, net.side_stream));
            continue;
        }
        if (i < net.waits.size())
            for (int pair : net.waits[i]) FHIP_CHECK_HIP(hipStreamWaitEvent(net.stream, net.events[2 * pair + 1], 0));
        const int rc = l->Forward(net.stream);
        if (rc) return rc;
    }
    return 0;
}

static int forward(Net& net)
{
    int rc = prepare(net);
    if (rc) return rc;
    if (!net.use_graph) return run_layers(net);
    if (!net.graph_exec)
    {
        hipGraph_t graph = nullptr;
        FHIP_CHECK_HIP(hipStreamBeginCapture(net.stream, hipStreamCaptureModeThreadLocal));
        rc = run_layers(net);
        const hipError_t e = hipStreamEndCapture(net.stream, &graph);
        if (rc)
        {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        FHIP_CHECK_HIP(e);
        const hipError_t ei = hipGraphInstantiate(&net.graph_exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        FHIP_CHECK_HIP(ei);
    }
    FHIP_CHECK_HIP(hipGraphLaunch(net.graph_exec, net.stream));
    return 0;
}

} // namespace fhip::net
