// feather/net.h -- C++ host class feather::Net over the MI355X runtime: the reference's public Net API
// (reference src/net.h:30-70, src/net.cpp) with the same method names, argument meaning and return codes, so code written
// against the reference links against libfeather_hip.so instead of libfeather.a:
//
//     feather::Net net;
//     net.LoadParam("model.param");  net.LoadWeights("model.bin");
//     ncnn::Mat in(w, h, c);  ...  net.FeedInput("data", in);   // net.h:44 (or the pointer forms below, with a batch)
//     net.Forward();
//     ncnn::Mat out;  net.Extract("prob", out);                  // net.h:50: host copy
//     float* dev; int n, c, h, w;  net.Extract("prob", &dev, &n, &c, &h, &w);   // net.h:48: pointer into the blob
//
// Differences, all forced by the GPU batch path:
//   * blobs live in HBM: Extract(name, float**, ...) returns a DEVICE pointer (use ExtractHost for a host copy);
//   * besides the reference's FeedInput(name, ncnn::Mat&) (N = 1, net.cpp:235-246) there are pointer forms with an explicit batch,
//     FeedPixels: ncnn's from_pixels_resize of a batch of uint8 images, done on the device (FeedPixelImages: images of mixed sizes,
//     pitches and ROIs);
//     and FeedYUV420sp: a batch of NV21 camera frames through either of the reference's yuv420sp chains, on the device;
//   * ExtractPixels: a blob that is an image comes back as uint8 pixels, ncnn's Mat::to_pixels_resize of every image of the batch done
//     on the device (libfeather_pixout.so: link it too when this method is used);
//   * Extract(name, ncnn::Mat&) copies channel by channel like the reference (net.cpp:281-296) -- but every channel, where the
//     reference copies channel 0 into all of them (its source pointer never advances); a batch > 1 comes back as n*c channels;
//   * public data members of the reference class are not mirrored: `blob_map` (std::map<std::string, Blob<float>*>, net.h:54)
//     exposes host Blob objects that do not exist here -- use Extract / LayerCount / the C-ABI introspection instead -- and the
//     feather::Layer / Blob classes (layer.h:29-88, blob.h) are internal to the device runtime;
//   * Forward only enqueues work on the net's HIP stream (SetStream); ExtractHost / Synchronize wait for it;
//   * SetFusion: 0 = none (what the reference actually does: TryFuse is never called),
//     1 = the reference's declared Conv-ReLU / BN-Scale-ReLU / InnerProduct-ReLU patterns (default), 2 = also fold
//     BatchNorm/Scale into the preceding convolution's weights, and run a squeeze-and-excitation block (global average Pooling, two
//     InnerProduct / 1x1 Convolution layers, Sigmoid / HardSigmoid, BinaryOp mul or two-bottom Scale, the residual Eltwise and its ReLU)
//     as one layer of libfeather_gate.so (FHIP_NET_ROUTE_GATE, feather_net.h);
//   * layer types beyond the reference's factory are loaded too: see feather_net.h's route codes (BinaryOp mul, Scale 0=-233, Swish and
//     HardSigmoid are the newest); Interp and HardSwish (FHIP_NET_ROUTE_RESAMPLE) and LRN (FHIP_NET_ROUTE_LRN) after
//     SetExtendedLayers(true); the SSD detection head (Permute, Flatten, Reshape, Normalize, PriorBox, DetectionOutput; feather_detect.h)
//     after SetDetection(true), its result through ExtractDetections; the YOLO heads after SetYolo(rows); Proposal, ROIPooling, ROIAlign
//     and PSROIPooling (feather_roi.h) after SetRoi(true), the ROIs through ExtractProposals; Padding, Crop and PixelShuffle
//     (feather_frame.h) after SetFrame(true); MemoryData, LayerNorm, GELU, MultiHeadAttention, the element-wise BinaryOp and the token-wise
//     InnerProduct (feather_attn.h) after SetTransformer(true) and SetDetection(true); LSTM, GRU and RNN (feather_rnn.h) after
//     SetRecurrent(true) and SetDetection(true).
// Header-only: every method forwards to the C-ABI in feather_hip/feather_net.h.
#pragma once

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "feather_hip/feather_net.h"
#include "feather_hip/feather_pixout.h"
#include "ncnn/mat.h"

namespace feather
{

// One row of a DetectionOutput top (ExtractDetections): ncnn's (label, score, xmin, ymin, xmax, ymax), the label as an int
struct Detection
{
    int label;
    float score, xmin, ymin, xmax, ymax;
};

// One row of a Proposal top (ExtractProposals): the box in image pixels and, where the scores were asked for, its foreground score
struct Roi
{
    float x1, y1, x2, y2, score;
};

class Net
{
  public:
    Net() : net_(NULL) { fhip_net_create(&net_); }
    ~Net()
    {
        if (net_) fhip_net_destroy(net_);
    }

    // Net::LoadParam / LoadWeights (net.cpp:54-233): 0 on success, negative on failure (-1 I/O, -200 unknown layer,
    // -300 topology error, -100 bad layer parameters), message in LastError().
    int LoadParam(const char* param_path) { return fhip_net_load_param(net_, param_path); }
    int LoadParam(FILE* fp) { return load_file(fp, true); }
    int LoadWeights(const char* weights_path) { return fhip_net_load_weights(net_, weights_path); }
    int LoadWeights(FILE* fp) { return load_file(fp, false); }
    int LoadParamMem(const char* text, size_t len) { return fhip_net_load_param_mem(net_, text, len); }
    int LoadWeightsMem(const void* data, size_t len) { return fhip_net_load_weights_mem(net_, data, len); }
    // the .bin image in device memory (the receive buffer of the RCCL weight broadcast, one rank per GPU)
    int LoadWeightsDevice(const void* device_data, size_t len) { return fhip_net_load_weights_device(net_, device_data, len); }

    // Net::FeedInput(const char*, ncnn::Mat&), net.h:44 / net.cpp:235-246 + Blob::CopyFromMat (blob.cpp:71-95): a host Mat of
    // shape (w, h, c), fp32, copied channel by channel (the Mat's channel stride may be padded to 16 bytes).  -1 for an unknown
    // blob name, -500 for a Mat that is not 3-D fp32.
    int FeedInput(const char* input_name, ncnn::Mat& in)
    {
        if (in.dims != 3 || in.elemsize != 4u || !in.data) return -500; // BAD DATA DIMENSION (blob.cpp:84)
        const size_t plane = (size_t)in.w * in.h;
        if (in.cstep == plane) return fhip_net_feed_input(net_, input_name, 1, in.c, in.h, in.w, (const float*)in.data, 0);
        std::string dense;
        dense.resize(plane * in.c * sizeof(float));
        for (int q = 0; q < in.c; ++q) memcpy(&dense[(size_t)q * plane * sizeof(float)], (const float*)in.data + in.cstep * q, plane * sizeof(float));
        return fhip_net_feed_input(net_, input_name, 1, in.c, in.h, in.w, (const float*)dense.data(), 0);
    }
    // The same with plain pointers and a batch.  `data` = n*c*h*w floats, NCHW dense, host memory.
    int FeedInput(const char* input_name, int c, int h, int w, const float* data) { return fhip_net_feed_input(net_, input_name, 1, c, h, w, data, 0); }
    int FeedInput(const char* input_name, int n, int c, int h, int w, const float* data) { return fhip_net_feed_input(net_, input_name, n, c, h, w, data, 0); }
    int FeedInputDevice(const char* input_name, int n, int c, int h, int w, const float* device_data)
    {
        return fhip_net_feed_input(net_, input_name, n, c, h, w, device_data, 1);
    }

    // uint8 images straight into the input blob, on the device (fhip_net_feed_pixels): ncnn's Mat::from_pixels_resize (+
    // substract_mean_normalize when mean / norm are given, cout values each) of `n` images [n][h][w][cin], host memory (one uint8 upload)
    // or, with FeedPixelsDevice, device memory.  The blob becomes [n][cout][target_h][target_w].  `type` is an ncnn::Mat::PIXEL_* code.
    int FeedPixels(const char* input_name, const unsigned char* pixels, int type, int w, int h, int target_w, int target_h,
                   const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_pixels(net_, input_name, 1, pixels, type, w, h, target_w, target_h, mean, norm, 0);
    }
    int FeedPixels(const char* input_name, int n, const unsigned char* pixels, int type, int w, int h, int target_w, int target_h,
                   const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_pixels(net_, input_name, n, pixels, type, w, h, target_w, target_h, mean, norm, 0);
    }
    int FeedPixelsDevice(const char* input_name, int n, const unsigned char* device_pixels, int type, int w, int h, int target_w, int target_h,
                         const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_pixels(net_, input_name, n, device_pixels, type, w, h, target_w, target_h, mean, norm, 1);
    }
    // A mixed-size batch straight into the input blob, on the device (fhip_net_feed_pixel_images): image i is `images[i]` (its own size,
    // row pitch and optional ROI), converted as ncnn's Mat::from_pixels_resize of a dense copy of its ROI (+ substract_mean_normalize).
    // The descriptors are host memory; their data is host memory (each ROI's rows uploaded) or, with FeedPixelImagesDevice, device
    // memory.  The blob becomes [n][cout][target_h][target_w].
    int FeedPixelImages(const char* input_name, int n, const fhip_pixel_image* images, int type, int target_w, int target_h,
                        const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_pixel_images(net_, input_name, n, images, type, target_w, target_h, mean, norm, 0);
    }
    int FeedPixelImagesDevice(const char* input_name, int n, const fhip_pixel_image* images, int type, int target_w, int target_h,
                              const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_pixel_images(net_, input_name, n, images, type, target_w, target_h, mean, norm, 1);
    }
    // NV21 (yuv420sp) camera frames straight into the input blob, on the device (fhip_net_feed_yuv420sp): `n` frames of w x h
    // (w*h*3/2 bytes each), host memory (one uint8 upload) or, with FeedYUV420spDevice, device memory.  type: ncnn::Mat::PIXEL_RGB,
    // PIXEL_RGB2BGR or PIXEL_RGB2GRAY.  resize_first = 1: the reference's resize_bilinear_yuv420sp -> yuv420sp2rgb -> from_pixels (even
    // target size, frame at least 4x4); 0: yuv420sp2rgb -> from_pixels_resize.  The blob becomes [n][cout][target_h][target_w].
    int FeedYUV420sp(const char* input_name, const unsigned char* yuv, int w, int h, int target_w, int target_h, int type,
                     int resize_first = 1, const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_yuv420sp(net_, input_name, 1, yuv, w, h, target_w, target_h, type, resize_first, mean, norm, 0);
    }
    int FeedYUV420sp(const char* input_name, int n, const unsigned char* yuv, int w, int h, int target_w, int target_h, int type,
                     int resize_first = 1, const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_yuv420sp(net_, input_name, n, yuv, w, h, target_w, target_h, type, resize_first, mean, norm, 0);
    }
    int FeedYUV420spDevice(const char* input_name, int n, const unsigned char* device_yuv, int w, int h, int target_w, int target_h, int type,
                           int resize_first = 1, const float* mean = NULL, const float* norm = NULL)
    {
        return fhip_net_feed_yuv420sp(net_, input_name, n, device_yuv, w, h, target_w, target_h, type, resize_first, mean, norm, 1);
    }

    int Forward() { return fhip_net_forward(net_); } // net.cpp:297-334

    // Net::Extract(name, float**, n, c, h, w), net.cpp:263-279; *output_ptr is a DEVICE pointer.
    int Extract(std::string blob_name, float** output_ptr, int* n, int* c, int* h, int* w)
    {
        return fhip_net_extract(net_, blob_name.c_str(), output_ptr, n, c, h, w);
    }
    // Net::Extract(std::string, ncnn::Mat&), net.h:50 / net.cpp:281-296: a host copy shaped (w, h, c) -- (w, h, n*c) for a batch.
    int Extract(std::string blob_name, ncnn::Mat& out)
    {
        float* dev = NULL;
        int n = 0, c = 0, h = 0, w = 0;
        int rc = fhip_net_extract(net_, blob_name.c_str(), &dev, &n, &c, &h, &w);
        if (rc) return rc;
        const size_t plane = (size_t)w * h, count = plane * c * n;
        out.create(w, h, c * n, 4u);
        if (out.empty() && count) return -1;
        if (out.cstep == plane) return fhip_net_extract_host(net_, blob_name.c_str(), (float*)out.data, count);
        std::string dense;
        dense.resize(count * sizeof(float));
        rc = fhip_net_extract_host(net_, blob_name.c_str(), (float*)&dense[0], count);
        if (rc) return rc;
        for (int q = 0; q < c * n; ++q) memcpy((float*)out.data + out.cstep * q, &dense[(size_t)q * plane * sizeof(float)], plane * sizeof(float));
        return 0;
    }
    // The blob as uint8 images, converted on the device (fhip_float_to_pixels, feather_pixout.h): image i of the batch becomes what the
    // reference's  m.substract_mean_normalize(mean, norm); m.to_pixels_resize(pixels_i, type, target_w, target_h)  makes of it, bit for
    // bit; `pixels` is [n][target_h][target_w][cn] in host memory (only these bytes cross the bus; the stream is synchronised) or, with
    // ExtractPixelsDevice, device memory (enqueued on the net's stream after Forward, no synchronisation).  type: ncnn::Mat::PIXEL_RGB,
    // PIXEL_BGR, PIXEL_GRAY, PIXEL_RGBA, PIXEL_RGB2BGR or PIXEL_BGR2RGB, whose channels must be the blob's; mean / norm: one value per
    // channel or NULL; pitch: bytes between output rows, 0 = dense.  *n_out (may be NULL) receives the batch.  Returns Extract's error for
    // a blob that cannot be extracted, FHIP_E_BADARG (message in LastPixelError()) for a bad type, size or channel count.
    int ExtractPixels(std::string blob_name, int* n_out, unsigned char* pixels, int type, int target_w, int target_h,
                      const float* mean = NULL, const float* norm = NULL, size_t pitch = 0)
    {
        return extract_pixels(blob_name, n_out, pixels, type, target_w, target_h, mean, norm, pitch, false);
    }
    int ExtractPixelsDevice(std::string blob_name, int* n_out, unsigned char* device_pixels, int type, int target_w, int target_h,
                            const float* mean = NULL, const float* norm = NULL, size_t pitch = 0)
    {
        return extract_pixels(blob_name, n_out, device_pixels, type, target_w, target_h, mean, norm, pitch, true);
    }
    int ExtractHost(std::string blob_name, float* host, size_t capacity_floats) { return fhip_net_extract_host(net_, blob_name.c_str(), host, capacity_floats); }

    int SetStream(void* hip_stream) { return fhip_net_set_stream(net_, hip_stream); }
    int SetFusion(int level) { return fhip_net_set_fusion(net_, level); }
    int SetGraph(bool on) { return fhip_net_set_graph(net_, on ? 1 : 0); }
    int SetTunedSelection(bool on) { return fhip_net_set_tuned_selection(net_, on ? 1 : 0); }
    // accept Convolution layers with dilation > 1 (libfeather_atrous.so) instead of refusing them; before LoadParam (feather_net.h)
    int SetDilated(bool on) { return fhip_net_set_dilated(net_, on ? 1 : 0); }
    // int8 Convolution / InnerProduct layers (ncnn's int8_scale_term) load and run through libfeather_qconv.so; before LoadParam
    int SetQuantized(bool on) { return fhip_net_set_quantized(net_, on ? 1 : 0); }
    // with SetQuantized: int8 convolutions with a requantised int8 output (int8_scale_term 101 .. 200) load, and the activation between
    // two int8 layers stays int8 on the device (libfeather_q8.so); before LoadParam (feather_net.h)
    int SetRequantized(bool on) { return fhip_net_set_requantized(net_, on ? 1 : 0); }
    // accept Interp and HardSwish layers (libfeather_resample.so) and LRN layers (libfeather_lrn.so) instead of refusing them; before
    // LoadParam (feather_net.h)
    int SetExtendedLayers(bool on) { return fhip_net_set_extended_layers(net_, on ? 1 : 0); }
    // accept the layers of ncnn's SSD detection head -- Permute, Flatten, Reshape, Normalize, PriorBox, DetectionOutput, Concat / Softmax along
    // any axis of a blob's rank (libfeather_detect.so) -- instead of refusing them; before LoadParam (feather_net.h)
    int SetDetection(bool on) { return fhip_net_set_detection(net_, on ? 1 : 0); }
    // The top of a DetectionOutput layer ([n][1][keep_top_k][6], zero rows past an image's count) as the detections of every image: a host
    // copy through Extract's pointer form and ExtractHost (synchronises).  Extract's error, or -100 if the blob has another shape.
    int ExtractDetections(std::string blob_name, std::vector<std::vector<Detection> >& out)
    {
        float* dev = NULL;
        int n = 0, c = 0, h = 0, w = 0;
        int rc = Extract(blob_name, &dev, &n, &c, &h, &w);
        if (rc) return rc;
        if (c != 1 || w != 6) return -100;
        std::vector<float> rows((size_t)n * h * 6);
        if ((rc = ExtractHost(blob_name, rows.data(), rows.size()))) return rc;
        out.assign(n, std::vector<Detection>());
        for (int i = 0; i < n; ++i)
            for (int r = 0; r < h; ++r)
            {
                const float* v = &rows[((size_t)i * h + r) * 6];
                if (!(v[0] > 0.f)) break;
                Detection d = {(int)v[0], v[1], v[2], v[3], v[4], v[5]};
                out[i].push_back(d);
            }
        return 0;
    }
    // accept the layers of ncnn's YOLO heads -- Reorg, YoloDetectionOutput, Yolov3DetectionOutput (libfeather_yolo.so) -- instead of refusing
    // them; `rows` is the height of the detection top ExtractDetections reads (the first `rows` detections of an image), 0 switches it off;
    // before LoadParam (feather_net.h)
    int SetYolo(int rows = 256) { return fhip_net_set_yolo(net_, rows); }
    // accept the layers of ncnn's two-stage detectors -- Proposal, ROIPooling, ROIAlign, PSROIPooling (libfeather_roi.so) -- instead of
    // refusing them; before LoadParam (feather_net.h)
    int SetRoi(bool on = true) { return fhip_net_set_roi(net_, on ? 1 : 0); }
    // accept ncnn's Padding, Crop and PixelShuffle (libfeather_frame.so) instead of refusing them; before LoadParam (feather_net.h)
    int SetFrame(bool on = true) { return fhip_net_set_frame(net_, on ? 1 : 0); }
    // accept the layers of a Vision Transformer encoder -- MemoryData, LayerNorm, GELU, MultiHeadAttention, the element-wise BinaryOp
    // (libfeather_attn.so), an InnerProduct once per token -- instead of refusing them; needs SetDetection(true) too; before LoadParam (feather_net.h)
    int SetTransformer(bool on = true) { return fhip_net_set_transformer(net_, on ? 1 : 0); }
    // accept ncnn's recurrent layers -- LSTM, GRU, RNN (libfeather_rnn.so) -- instead of refusing them; needs SetDetection(true) too; before
    // LoadParam (feather_net.h)
    int SetRecurrent(bool on = true) { return fhip_net_set_recurrent(net_, on ? 1 : 0); }
    // The tops of a Proposal layer ([n][R][1][4], sentinel rows (0, 0, -1, -1) past an image's count, and optionally the scores [n][R][1][1])
    // as the ROIs of every image: a host copy through Extract's pointer form and ExtractHost (synchronises).  Extract's error, or -100 if a
    // blob has another shape.  scores_blob "" asks for none.
    int ExtractProposals(std::string rois_blob, std::vector<std::vector<Roi> >& out, std::string scores_blob = "")
    {
        float* dev = NULL;
        int n = 0, c = 0, h = 0, w = 0;
        int rc = Extract(rois_blob, &dev, &n, &c, &h, &w);
        if (rc) return rc;
        if (h != 1 || w != 4) return -100;
        std::vector<float> rows((size_t)n * c * 4), scores;
        if ((rc = ExtractHost(rois_blob, rows.data(), rows.size()))) return rc;
        if (!scores_blob.empty())
        {
            int sn = 0, sc = 0, sh = 0, sw = 0;
            if ((rc = Extract(scores_blob, &dev, &sn, &sc, &sh, &sw))) return rc;
            if (sn != n || sc != c || sh != 1 || sw != 1) return -100;
            scores.resize((size_t)n * c);
            if ((rc = ExtractHost(scores_blob, scores.data(), scores.size()))) return rc;
        }
        out.assign(n, std::vector<Roi>());
        for (int i = 0; i < n; ++i)
            for (int r = 0; r < c; ++r)
            {
                const float* v = &rows[((size_t)i * c + r) * 4];
                if (!(v[2] >= v[0])) break;
                Roi roi = {v[0], v[1], v[2], v[3], scores.empty() ? 0.f : scores[(size_t)i * c + r]};
                out[i].push_back(roi);
            }
        return 0;
    }
    int SetConcurrency(bool on) { return fhip_net_set_concurrency(net_, on ? 1 : 0); }
    int SetColpass(int mode) { return fhip_net_set_colpass(net_, mode); } // 0 never, 1 where M is HBM-bound (default), 2 wherever accepted
    int SetSubBatches(int replicas) { return fhip_net_set_sub_batches(net_, replicas); } // before LoadParam (feather_net.h)
    int LayerCount() { return fhip_net_layer_count(net_); }
    static const char* LastError() { return fhip_last_error(); }
    static const char* LastPixelError() { return fhip_pixout_last_error(); } // ExtractPixels: the output library keeps its own message
    fhip_net* handle() { return net_; }

  private:
    Net(const Net&);
    Net& operator=(const Net&);
    int extract_pixels(const std::string& blob_name, int* n_out, unsigned char* pixels, int type, int target_w, int target_h,
                       const float* mean, const float* norm, size_t pitch, bool on_device)
    {
        float* dev = NULL;
        int n = 0, c = 0, h = 0, w = 0;
        void* stream = NULL;
        int rc = fhip_net_extract(net_, blob_name.c_str(), &dev, &n, &c, &h, &w); // gathers sub-batch replicas on the net's stream
        if (rc) return rc;
        rc = fhip_net_get_stream(net_, &stream);
        if (rc) return rc;
        const int cn = fhip_pixout_channels(type);
        if (cn < 0) return cn;
        if (cn != c) return FHIP_E_BADARG; // the blob is not an image of this type
        if (n_out) *n_out = n;
        return on_device ? fhip_float_to_pixels(pixels, pitch, dev, n, type, w, h, target_w, target_h, mean, norm, stream)
                         : fhip_float_to_pixels_host(pixels, pitch, dev, n, type, w, h, target_w, target_h, mean, norm, stream);
    }
    int load_file(FILE* fp, bool param)
    {
        if (!fp) return -1;
        std::string buf;
        char chunk[1 << 16];
        size_t got;
        if (param) fseek(fp, 0, SEEK_SET); // ChkParamHeader rewinds too (utils.cpp:29)
        while ((got = fread(chunk, 1, sizeof(chunk), fp)) > 0) buf.append(chunk, got);
        return param ? fhip_net_load_param_mem(net_, buf.data(), buf.size()) : fhip_net_load_weights_mem(net_, buf.data(), buf.size());
    }
    fhip_net* net_;
};

} // namespace feather
