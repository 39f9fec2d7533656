// net_model.h -- the readers of ncnn's .param values (ParamDict) and .bin weights (ModelBin); they know no layer.
#pragma once
#include "net_side.h"

namespace fhip::net
{

// ---- ncnn ParamDict (ncnn/paramdict.cpp:92-174): "id=value" pairs, value is float iff it contains '.' or 'e' -----
struct ParamDict
{
    static const int kMax = 32; // NCNN_MAX_PARAM_COUNT is 20
    struct Entry
    {
        bool loaded = false;
        uint32_t bits = 0; // union { int i; float f; } exactly like the reference
        std::vector<float> array;
    } e[kMax];

    void clear()
    {
        for (auto& x : e) x = Entry();
    }
    int get(int id, int def) const
    {
        if (id < 0 || id >= kMax || !e[id].loaded) return def;
        int v;
        memcpy(&v, &e[id].bits, 4);
        return v;
    }
    float get(int id, float def) const
    {
        if (id < 0 || id >= kMax || !e[id].loaded) return def;
        float v;
        memcpy(&v, &e[id].bits, 4);
        return v;
    }
    bool has_array(int id) const { return id >= 0 && id < kMax && e[id].loaded && !e[id].array.empty(); }

    static bool is_float(const std::string& s)
    {
        for (char ch : s)
            if (ch == '.' || ch == 'e' || ch == 'E') return true;
        return false;
    }
    // `tok` is one whitespace-delimited token "id=value" or "-233xx=len,v0,v1,..."; returns false if it is not a pair.
    static bool looks_like_pair(const std::string& tok)
    {
        size_t i = 0;
        if (i < tok.size() && tok[i] == '-') ++i;
        const size_t d0 = i;
        while (i < tok.size() && isdigit((unsigned char)tok[i])) ++i;
        return i > d0 && i < tok.size() && tok[i] == '=';
    }
    int parse(const std::string& tok)
    {
        const size_t eq = tok.find('=');
        // a file may hold any digits: the id is read wide, and its range is checked before any arithmetic on it
        errno = 0;
        const long long raw_id = strtoll(tok.substr(0, eq).c_str(), nullptr, 10);
        const std::string val = tok.substr(eq + 1);
        const bool is_array = raw_id <= -23300;
        if (errno == ERANGE || raw_id <= -23300 - kMax || raw_id >= kMax || (raw_id < 0 && !is_array))
            return failf(FHIP_E_BADARG, "param id %.24s out of range", tok.c_str());
        const long long wide_id = is_array ? -raw_id - 23300 : raw_id;
        const int id = (int)wide_id;
        if (is_array)
        {
            std::vector<std::string> parts;
            size_t a = 0;
            while (a <= val.size())
            {
                const size_t b = val.find(',', a);
                parts.push_back(val.substr(a, b == std::string::npos ? std::string::npos : b - a));
                if (b == std::string::npos) break;
                a = b + 1;
            }
            const int len = atoi(parts[0].c_str());
            if (len < 0 || parts.size() != (size_t)len + 1) return failf(NET_E_IO, "ParamDict read array element fail"); // paramdict.cpp:124-128
            e[id].array.resize(len);
            for (int j = 0; j < len; ++j) e[id].array[j] = (float)atof(parts[j + 1].c_str());
        }
        else
        {
            if (val.empty()) return failf(NET_E_IO, "ParamDict read value fail"); // paramdict.cpp:153-157
            if (is_float(val))
            {
                const float f = (float)atof(val.c_str());
                memcpy(&e[id].bits, &f, 4);
            }
            else
            {
                const int i = atoi(val.c_str());
                memcpy(&e[id].bits, &i, 4);
            }
        }
        e[id].loaded = true;
        return 0;
    }
};

// ---- ncnn ModelBin (ncnn/modelbin.cpp:47-197) over a memory image of the .bin ---------------------------------
struct ModelBin
{
    const unsigned char* p;
    const unsigned char* end;

    static float half_to_float(uint16_t h)
    {
        const uint32_t sign = (uint32_t)(h >> 15) << 31;
        int exp = (h >> 10) & 0x1f;
        uint32_t man = h & 0x3ff;
        uint32_t bits;
        if (exp == 0)
        {
            if (man == 0)
                bits = sign;
            else
            {
                exp = 1;
                while (!(man & 0x400))
                {
                    man <<= 1;
                    --exp;
                }
                man &= 0x3ff;
                bits = sign | ((uint32_t)(exp + 112) << 23) | (man << 13);
            }
        }
        else if (exp == 31)
            bits = sign | 0x7f800000u | (man << 13);
        else
            bits = sign | ((uint32_t)(exp + 112) << 23) | (man << 13);
        float f;
        memcpy(&f, &bits, 4);
        return f;
    }
    bool take(void* dst, size_t bytes)
    {
        if ((size_t)(end - p) < bytes) return false;
        if (dst) memcpy(dst, p, bytes);
        p += bytes;
        return true;
    }
    // The int8 weights of a quantised layer (tag 0x000D4B38, then w bytes padded to 4: modelbin.cpp:92-109 reads them so).  Weights under
    // any other tag are refused: this runtime does not quantise at load.  load() below keeps refusing the tag for every fp32 caller.
    int load_int8(size_t w, std::vector<signed char>& out)
    {
        out.clear();
        unsigned char f[4];
        if (!take(f, 4)) return failf(NET_E_SHAPE, "ModelBin read flag_struct failed");
        uint32_t tag;
        memcpy(&tag, f, 4);
        if (tag != 0x000D4B38u) return failf(FHIP_E_UNSUPPORTED, "an int8 layer (int8_scale_term) needs int8 weights (tag 0x000D4B38), found tag 0x%08X: weights are not quantised at load", tag);
        const size_t rest = (size_t)(end - p);
        // the count is a product of file values: checked against the rest of the file before anything of that size is allocated
        if (w > rest || (w + 3) / 4 * 4 > rest) return failf(NET_E_SHAPE, "ModelBin read int8_weights failed (file too short for %zu weights padded to 4 bytes)", w);
        out.assign(reinterpret_cast<const signed char*>(p), reinterpret_cast<const signed char*>(p) + w);
        p += (w + 3) / 4 * 4;
        return 0;
    }
    // type 0: 4-byte tag then payload (raw fp32 / fp16 / 256-entry table); type 1: raw fp32 (modelbin.cpp:52-189)
    int load(size_t w, int type, std::vector<float>& out)
    {
        // every payload form holds at least one byte per weight: a count the rest of the file cannot hold is refused before anything of
        // that size is allocated (counts are products of file values: negative ones arrive here as huge ones)
        if (w > (size_t)(end - p))
        {
            out.clear();
            return failf(NET_E_SHAPE, "ModelBin read weight_data failed (file too short for %zu weights)", w);
        }
        out.assign(w, 0.f);
        if (type == 1)
        {
            if (!take(out.data(), w * 4)) return failf(NET_E_SHAPE, "ModelBin read weight_data failed (file too short)");
            return 0;
        }
        if (type != 0) return failf(NET_E_SHAPE, "ModelBin load type %d not implemented", type);
        unsigned char f[4];
        if (!take(f, 4)) return failf(NET_E_SHAPE, "ModelBin read flag_struct failed");
        uint32_t tag;
        memcpy(&tag, f, 4);
        const unsigned flag = f[0] + f[1] + f[2] + f[3];
        if (tag == 0x01306B47u) // fp16 payload, padded to 4 bytes
        {
            const size_t bytes = (w * 2 + 3) / 4 * 4;
            if ((size_t)(end - p) < bytes) return failf(NET_E_SHAPE, "ModelBin read float16_weights failed");
            for (size_t i = 0; i < w; ++i)
            {
                uint16_t h;
                memcpy(&h, p + 2 * i, 2);
                out[i] = half_to_float(h);
            }
            p += bytes;
            return 0;
        }
        if (tag == 0x000D4B38u) return failf(FHIP_E_UNSUPPORTED, "int8 weights are not supported (conv_layer.h:50-55 rejects them too)");
        if (tag == 0x0002C056u)
        {
            if (!take(out.data(), w * 4)) return failf(NET_E_SHAPE, "ModelBin read weight_data failed");
            return 0;
        }
        if (flag != 0) // 256-entry codebook + one byte per weight, padded to 4 bytes
        {
            float table[256];
            if (!take(table, sizeof(table))) return failf(NET_E_SHAPE, "ModelBin read quantization_value failed");
            const size_t bytes = (w + 3) / 4 * 4;
            if ((size_t)(end - p) < bytes) return failf(NET_E_SHAPE, "ModelBin read index_array failed");
            for (size_t i = 0; i < w; ++i) out[i] = table[p[i]];
            p += bytes;
            return 0;
        }
        if (!take(out.data(), w * 4)) return failf(NET_E_SHAPE, "ModelBin read weight_data failed (file too short)");
        return 0;
    }
};

} // namespace fhip::net
