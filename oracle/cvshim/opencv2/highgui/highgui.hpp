// stand-in for the four window / file calls of Flow::ShowImage (rw_flow.cpp:334-340): no-ops (see ../core/core.hpp)
#ifndef BBME_CVSHIM_HIGHGUI_HPP
#define BBME_CVSHIM_HIGHGUI_HPP
#include "../core/core.hpp"
namespace cv {
inline void namedWindow(const std::string &) {}
inline void imshow(const std::string &, const Mat &) {}
inline bool imwrite(const std::string &, const Mat &) { return true; }
inline int waitKey(int) { return 0; }
}
#endif
