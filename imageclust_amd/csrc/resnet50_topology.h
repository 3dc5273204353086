// resnet50_topology.h -- the 53 convolution records of ResNet50-v1 in canonical order (stem; per bottleneck c1, c2, c3 and, for block 0, the
// downsample branch).  Plain C++ with no HIP in it: model.hip, onnx_reader.hip and tests/conv_select_main.cpp all read this one copy.
#pragma once
#include "../../include/icl_model_format.h"

inline int resnet50_topology(icl_conv_rec *out /* [ICL_RESNET50_NCONV] */)
{
    static const int nblocks[4] = {3, 4, 6, 3};
    int n = 0;
    out[n++] = icl_conv_rec{3, 64, 7, 2, 3, 224, 112, 0, 0, 0};
    int h = 56, cin = 64;
    for (int s = 0; s < 4; ++s) {
        const int cout = 256 << s, mid = cout / 4;
        for (int b = 0; b < nblocks[s]; ++b) {
            const int stride = (b == 0 && s > 0) ? 2 : 1, ho = h / stride;
            out[n++] = icl_conv_rec{cin, mid, 1, stride, 0, h, ho, 1, s + 1, b};
            out[n++] = icl_conv_rec{mid, mid, 3, 1, 1, ho, ho, 2, s + 1, b};
            out[n++] = icl_conv_rec{mid, cout, 1, 1, 0, ho, ho, 3, s + 1, b};
            if (b == 0) out[n++] = icl_conv_rec{cin, cout, 1, stride, 0, h, ho, 4, s + 1, b};
            cin = cout;
            h = ho;
        }
    }
    return n;
}
