// stand-in: the reference includes this header and uses nothing from it (see ../core/core.hpp)
#include "../core/core.hpp"
