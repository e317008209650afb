#pragma once
#include "../../../df_min.h"  // test-only stand-in, see df_min.h
