// Blackjack-v1 with natural = False, sab = False and the infinite deck (gymnasium's toy_text/blackjack.py; the reference has no such env): the host-side class
// of PPO_ENV_BLACKJACK, the CPU twin of the device env.  It computes on the CPU from the same statement -- include/ppo_hip.h: the cards drawn from Philox keyed
// by state words, the hit, the dealer's play-out, the deal, the three one-hot groups of the observation -- in integers, so a state stepped here and by
// ppo_env_transition(PPO_ENV_BLACKJACK, ..) gives the same numbers (tests/test_gpu_blackjack_facade.py).  It needs no device and no library.  The randomness
// of an episode rides in its state: {hand, n, k0, k1}, hand = t + 32 * ace + 64 * show, the index of the next card and the episode's key.
#pragma once
#include <array>
#include <cstdint>
#include <tuple>
#include <vector>

class Blackjack {
  public:
    static constexpr int OBS = 45;             // gymnasium's flattened Tuple(Discrete(32), Discrete(11), Discrete(2))
    static constexpr int DEALER_DRAWS = 10;    // the most cards a dealer draws from any two-card start

    std::vector<float> state;      // {hand, n, k0, k1}: hand = t + 32 * ace + 64 * show (t in 2..31, ace in 0..1, show in 1..10); n, k0, k1 in 0..2^24-1
    int64_t episode_length;
    float episode_reward;

    explicit Blackjack(int64_t seed = 1, int64_t env_index = 0);
    // {observation (45 floats: sum at [0..31], 32 + show at [32..42], 43 + usable at [43..44]), reward (-1, 0 or 1), terminated, truncated (never: the
    // algorithm counts max_episode_steps)}; action in 0..1 (stick, hit), clamped
    std::tuple<std::vector<float>, float, bool, bool> step(int64_t action);
    std::vector<float> reset();    // a fresh key and its deal; the observation of the new state
    std::vector<float> observation() const;

    // the bare step: st[4] (components converted and clamped into their ranges) -> next state in place; returns the reward; `drawn` (optional): the cards the
    // dealer drew
    static float transition(float* st, int action, bool& terminated, int* drawn = nullptr);
    static void observe(const float* st, float* obs);
    static int card(uint32_t word);                                  // min(1 + ((uint64(word) * 13) >> 32), 10)
    static int cardAt(uint32_t k0, uint32_t k1, uint32_t index);      // card number `index` of the episode with key (k0, k1)
    static std::array<uint32_t, 4> philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3);

  private:
    int64_t m_seed, m_env_index, m_resets = 0;
};
