#include "FrozenLake.h"

#include <stdexcept>

namespace {
constexpr int WORD_MAX = (1 << 24) - 1;
constexpr uint64_t HOLES_4 = 0x18a0ull;                 // SFFF FHFH FFFH HFFG: {5, 7, 11, 12}
constexpr uint64_t HOLES_8 = 0x0852460820080000ull;     // gymnasium's 8x8: {19, 29, 35, 41, 42, 46, 49, 52, 54, 59}

int clampi(float v, int hi) { return v >= 0.0f ? (v >= static_cast<float>(hi) ? hi : static_cast<int>(v)) : 0; }   // a NaN becomes 0
bool terminal(int side, int cell) { return cell == side * side - 1 || FrozenLake::isHole(side, cell); }
}  // namespace

bool FrozenLake::isHole(int side, int cell) { return (((side == 8 ? HOLES_8 : HOLES_4) >> cell) & 1ull) != 0; }

std::array<uint32_t, 4> FrozenLake::philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0, p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
        const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0, n1 = static_cast<uint32_t>(p1);
        const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1, n3 = static_cast<uint32_t>(p0);
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return { c0, c1, c2, c3 };
}

float FrozenLake::transition(int side, float* st, int action, bool& terminated) {
    const int S = side * side;
    int cell = clampi(st[0], S - 1);
    const int j = clampi(st[1], WORD_MAX), k0 = clampi(st[2], WORD_MAX), k1 = clampi(st[3], WORD_MAX);
    const int a = action < 0 ? 0 : (action > 3 ? 3 : action);
    float reward = 0.0f;
    terminated = true;
    if (!terminal(side, cell)) {
        const std::array<uint32_t, 4> w = philox4x32_10(static_cast<uint32_t>(k0), static_cast<uint32_t>(k1), static_cast<uint32_t>(j >> 2), 0u, 0u, 0x20u);
        const int d = static_cast<int>((static_cast<uint64_t>(w[static_cast<size_t>(j & 3)]) * 3u) >> 32);
        const int eff = (a + d + 3) & 3;   // gym's [(a - 1) % 4, a, (a + 1) % 4]; 0 left, 1 down, 2 right, 3 up
        int row = cell / side, col = cell % side;
        if (eff == 0) col = col > 0 ? col - 1 : 0;
        else if (eff == 1) row = row < side - 1 ? row + 1 : side - 1;
        else if (eff == 2) col = col < side - 1 ? col + 1 : side - 1;
        else row = row > 0 ? row - 1 : 0;
        cell = row * side + col;
        terminated = terminal(side, cell);
        reward = cell == S - 1 ? 1.0f : 0.0f;
    }
    st[0] = static_cast<float>(cell);
    st[1] = static_cast<float>(j < WORD_MAX ? j + 1 : WORD_MAX);
    st[2] = static_cast<float>(k0);
    st[3] = static_cast<float>(k1);
    return reward;
}

void FrozenLake::observe(int side, const float* st, float* obs) {
    const int S = side * side;
    for (int k = 0; k < S; k++) obs[k] = 0.0f;
    obs[clampi(st[0], S - 1)] = 1.0f;
}

FrozenLake::FrozenLake(int side, int64_t seed, int64_t env_index)
    : state(4, 0.0f), episode_length(0), episode_reward(0.0f), m_side(side), m_seed(seed), m_env_index(env_index) {
    if (side != 4 && side != 8) throw std::invalid_argument("FrozenLake: side must be 4 (FrozenLake-v1) or 8 (FrozenLake8x8-v1)");
}

std::vector<float> FrozenLake::observation() const {
    std::vector<float> obs(static_cast<size_t>(m_side * m_side));
    observe(m_side, state.data(), obs.data());
    return obs;
}

std::tuple<std::vector<float>, float, bool, bool> FrozenLake::step(int64_t action) {
    bool terminated = false;
    const int a = action < 0 ? 0 : (action > 3 ? 3 : static_cast<int>(action));
    const float reward = transition(m_side, state.data(), a, terminated);
    episode_length += 1;
    episode_reward += reward;
    return { observation(), reward, terminated, false };
}

// The device's reset map: reset number k of env e under `seed` draws philox4x32_10(seed; e, k, 0, 1) and keeps the top 24 bits of its first two words as the key
std::vector<float> FrozenLake::reset() {
    const uint64_t s = static_cast<uint64_t>(m_seed);
    const std::array<uint32_t, 4> w = philox4x32_10(static_cast<uint32_t>(s), static_cast<uint32_t>(s >> 32), static_cast<uint32_t>(m_env_index),
                                                    static_cast<uint32_t>(m_resets++), 0u, 1u);
    state = { 0.0f, 0.0f, static_cast<float>(w[0] >> 8), static_cast<float>(w[1] >> 8) };
    episode_length = 0;
    episode_reward = 0.0f;
    return observation();
}
