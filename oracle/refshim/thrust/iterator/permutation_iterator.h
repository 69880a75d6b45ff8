/* stand-in: everything the reference kernels use of thrust is in stub.h */
#include <thrust/stub.h>
