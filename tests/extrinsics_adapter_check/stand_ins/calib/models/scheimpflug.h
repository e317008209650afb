#pragma once
#include "../../ext_min.h"  // test-only stand-in, see ext_min.h
