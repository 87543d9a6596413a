// Shared by the Haar detector (ef_haar.hip) and the rectangle grouping (ef_haar_group.hip).
#pragma once

#include "ef_internal.hpp"

namespace ef {

struct HaarLayer {
  int w, h, nx, ny, step;
  float scale;
  int64_t pix_off, ii_off, res_off;
};
struct HaarCand {
  int layer, y, x;
  float vnf;  // the window's normalisation factor (stage 0's haar_norm), carried along the lists
};

// Most rectangles one grouping takes (include/eigenface.h EF_HAAR_GROUP_MAX).
constexpr int kHaarGroupMax = EF_HAAR_GROUP_MAX;

// Scratch of one grouping of at most maxc rectangles (device pointers).
struct HaarGroupWs {
  int4* rect;                // [maxc] {x, y, w, h} in list order
  unsigned long long* key;   // [maxc] the order OpenCV lists the rectangles in: (layer, y, x), or the list index
  int* parent;               // [maxc] union-find forest; a parent's key is smaller than its child's
  int* root;                 // [maxc] the component's member of smallest key
  int4* cls_rect;            // [maxc] averaged rectangle per class, classes in OpenCV's order
  int* cls_cnt;              // [maxc] members per class
  int* keep;                 // [maxc] 1: the class passes both filters
  int* count;                // [0] classes, [1] status bits, [2] the rectangle count of ef_haar_group
};
inline HaarGroupWs carve_haar_group_ws(Carve& cv, size_t maxc) {
  return HaarGroupWs{cv.take<int4>(maxc), cv.take<unsigned long long>(maxc), cv.take<int>(maxc), cv.take<int>(maxc),
                     cv.take<int4>(maxc), cv.take<int>(maxc),                cv.take<int>(maxc), cv.take<int>(4)};
}

// cv::groupRectangles(min_neighbors, 0.2) of at most maxc rectangles, queued on s (six launches,
// no host wait).  cand non-null: the rectangles are the detector's candidates cand[*ncount]
// (HaarCand -> rectangle with ef_haar_detect's arithmetic), in OpenCV's (layer, y, x) order
// whatever order the list holds them in.  cand null: ws.rect holds n_host rectangles in list
// order (ncount is not read).  A count above maxc groups nothing and sets EF_HAAR_SCAN_OVERFLOW.
// rects_out[max_rects][4] takes the first max_rects grouped rectangles, zeros behind them;
// head (optional) the header, n_rects_out (optional) the count alone.
hipError_t launch_haar_group(hipStream_t s, const HaarCand* cand, const HaarLayer* layers, int ww, int wh,
                             const int* ncount, int n_host, int maxc, int min_neighbors, const HaarGroupWs& ws,
                             ef_haar_scan_head* head, int* n_rects_out, int* rects_out, int max_rects);

}  // namespace ef
