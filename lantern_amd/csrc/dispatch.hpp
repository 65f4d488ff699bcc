// dispatch.hpp -- host-side dispatch of a kernel template on (metric code, lanes per row).
#pragma once
#include "device_common.hpp"

// CALL(MM, G) for the lanes per row G_
#define LGPU_DISPATCH_G(G_, MM, CALL)                                                                      \
    switch(G_) { case 64: CALL(MM, 64); break; case 32: CALL(MM, 32); break; case 16: CALL(MM, 16); break; default: CALL(MM, 8); }

// dispatch on (metric, lanes per row)
#define LGPU_DISPATCH(metric, chunks, CALL)                                   \
    do {                                                                      \
        const int G_ = group_lanes_for(chunks);                               \
        switch(metric) {                                                      \
            case M_L2SQ: LGPU_DISPATCH_G(G_, M_L2SQ, CALL) break;             \
            case M_COS: LGPU_DISPATCH_G(G_, M_COS, CALL) break;               \
            case M_HAMMING: LGPU_DISPATCH_G(G_, M_HAMMING, CALL) break;       \
            case M_COS_B1: LGPU_DISPATCH_G(G_, M_COS_B1, CALL) break;         \
            case M_L2SQ_F16: LGPU_DISPATCH_G(G_, M_L2SQ_F16, CALL) break;     \
            case M_COS_F16: LGPU_DISPATCH_G(G_, M_COS_F16, CALL) break;       \
            case M_L2SQ_I8: LGPU_DISPATCH_G(G_, M_L2SQ_I8, CALL) break;       \
            case M_COS_I8: LGPU_DISPATCH_G(G_, M_COS_I8, CALL) break;         \
            default: return hipErrorInvalidValue;                             \
        }                                                                     \
    } while(0)

// a compact pq index, rows decoded on the fly (device_common.hpp PqdRow): the two decoding metrics, G by the DECODED row
#define PQD_G(metric, chunks, CALL)                                           \
    do {                                                                      \
        const int G_ = group_lanes_for(chunks);                               \
        if(metric == M_L2SQ_PQD) LGPU_DISPATCH_G(G_, M_L2SQ_PQD, CALL)        \
        else if(metric == M_COS_PQD) LGPU_DISPATCH_G(G_, M_COS_PQD, CALL)     \
        else return hipErrorInvalidValue;                                     \
    } while(0)
