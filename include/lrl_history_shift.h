/* lrl_history_shift.h - the history shift done by the rollout act, part of liblrl's C ABI (include/lrl.h includes this
 * file; lrl_sim, lrl_ppo_net, lrl_rollout_store and the LRL_E_* codes are declared there).  Appended entry points: no
 * struct or function that existed before changes, so LRL_ABI_VERSION stays.
 *
 * HistoryWrapper.step moves every env's history row left by one observation and appends the step's observation.  In a
 * rollout the act has just read those rows to copy them into the rollout storage, so it can store them a second time,
 * one slot to the left, and the sim's own shift launch (shift_history_kernel) has nothing left to do. */
#ifndef LRL_HISTORY_SHIFT_H_
#define LRL_HISTORY_SHIFT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* lrl_ppo_act that also performs the HistoryWrapper.step shift of the rows it copies into storage: with hist_shift ==
 * hist (writable) every row r < n becomes hist[r][:H - hist_slot] = hist[r][hist_slot:] in place (H = store->hist_dim,
 * hist_slot the observation width, which divides H); the newest slot hist[r][H - hist_slot:] is not written and
 * store->hist receives the unshifted row.  Needs `store` with a history array.  hist_shift == NULL is lrl_ppo_act.
 * lrl_sim_history_preshifted tells the next lrl_sim_step which rows need no shift. */
int32_t lrl_ppo_act_shift(const lrl_ppo_net* net, const float* params, const float* obs, const float* priv,
                          const float* hist, int32_t n, const float* eps, uint64_t seed, uint64_t counter,
                          int64_t row_offset, float* actions, float* mu, float* values, float* logp,
                          const lrl_rollout_store* store, int32_t store_row, void* workspace, void* stream,
                          float* hist_shift, int32_t hist_slot);

/* One-shot: rows [0, rows) of the history buffer are already shifted (lrl_ppo_act_shift did it), so the next
 * lrl_sim_step with LRL_STEP_HISTORY shifts rows [rows, num_envs) only (nothing when rows == num_envs) and clears the
 * count.  rows < 0 or rows > num_envs is LRL_E_INVALID. */
int32_t lrl_sim_history_preshifted(lrl_sim* sim, int32_t rows);

#ifdef __cplusplus
}
#endif

#endif /* LRL_HISTORY_SHIFT_H_ */
