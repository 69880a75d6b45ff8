/* stand-in: everything the reference kernels use of OpenCV is in cvshim.hpp */
#include <opencv2/cvshim.hpp>
