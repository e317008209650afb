#pragma once
#include "../../ls_min.h"  // test-only stand-in, see ls_min.h
