// The tuning table (WM_TUNE_KEYS, wm_kernels.h) and wm_set_tuning: nothing else, so that a planner can be linked without the orchestrator.
#include "wm_kernels.h"

#include <string.h>

#define WM_TUNE_UNSET(name_, key_) -1,
#define WM_TUNE_NAME(name_, key_) key_,
int wm_tuning[WM_TUNE_COUNT] = {WM_TUNE_KEYS(WM_TUNE_UNSET)};
static const char* const wm_tuning_keys[WM_TUNE_COUNT] = {WM_TUNE_KEYS(WM_TUNE_NAME)};

extern "C" int wm_set_tuning(const char* key, int value) {
  for (int i = 0; i < WM_TUNE_COUNT; ++i)
    if (key && strcmp(key, wm_tuning_keys[i]) == 0) { wm_tuning[i] = value; return 0; }
  return -1;
}
