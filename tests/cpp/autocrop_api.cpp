// autocrop_api.cpp — compile test of the declarations of include/prl/autoCrop.h against OpenCV's declared API (tests/cpp/opencv_api,
// found through -I; built with -fsyntax-only -DPRL_REQUIRE_OPENCV by tests/test_contour_cpu.py).  The declaration-only headers
// carry cv::Point_ but not the typedef the reference's header spells, so it is declared here as OpenCV does
// (opencv2/core/types.hpp); the pointers below then hold the reference's signatures (src/border_detection/autoCrop.h:42-53) letter
// for letter, and its defaults: none.
#include <opencv2/core/core.hpp>

namespace cv {
typedef Point_<float> Point2f;
}

#include "autoCrop.h"

#include <vector>

namespace {

bool (*const document_contour)(cv::Mat& inputImage, const double scaleX, const double scaleY, std::vector<cv::Point2f>& resultContour) =
    &prl::documentContour;
bool (*const auto_crop)(cv::Mat& inputImage, cv::Mat& outputImage) = &prl::autoCrop;

bool caller(cv::Mat& page, cv::Mat& cropped)
{
    std::vector<cv::Point2f> contour;
    const bool found = prl::documentContour(page, -1, -1, contour) && document_contour(page, -1, -1, contour);
    return found && prl::autoCrop(page, cropped) && auto_crop(page, cropped);
}

}  // namespace

int main()
{
    cv::Mat a, b;
    return caller(a, b) ? 0 : 1;
}
